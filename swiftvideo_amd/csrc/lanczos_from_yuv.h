// lanczos_from_yuv.h — what chv_scale_lanczos_from_yuv / chv_scale_lanczos_from_yuv_batch (chipvideo.cpp) and their kernel unit
// (kernels_lanczos_from_yuv.hip.cpp) share.
//
// The decoder side's rendition in one launch: an NV12 or y420p picture becomes a BGRA or RGBA plane of another size.
// The logical planes Y, Cb and Cr are each resampled to the TARGET's size as chv_scale_lanczos resamples a 1-component plane, rounded to
// codes, and the three codes of a pixel go through the integer matrix of section 4.2.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"
#include "lanczos_planar.h"

namespace chv {

struct LanczosFromYuvJob {
    // luma: the tables of (iw, ow) and (ih, oh); chroma: of (cw, ow) and (ch, oh), shared by Cb and Cr — device memory that stays valid
    // until the launch has run
    LanczosPlaneTables luma, chroma;
    // picture 0's planes; every picture of a batch has these sizes.  src[0]: Y; src[1]: the CbCr plane (NV12) or Cb (y420p); src[2]: Cr (y420p)
    DPlane dst, src[kLanczosPlanarMaxPlanes];
    int32_t src_planes;                                // 2: NV12, 3: y420p
    int32_t rgba;                                      // the target's byte order: 0 B, G, R, 255; 1 R, G, B, 255
    int32_t yoff, cy, crv, cgu, cgv, cbu;              // section 4.2's row for the call's colourspace
    // batch != nullptr: n_pictures pictures of 1 + src_planes planes each, picture i's target at batch[i * (1 + src_planes)], its source
    // planes behind it, in memory the device can read that stays unchanged until the launch has run.  nullptr: the one picture above
    // travels in the launch's arguments.
    const DPlane *batch;
    int32_t n_pictures;
};

// One launch.  hipErrorInvalidValue for a logical plane whose own (in, out) sizes chv_scale_lanczos refuses (nothing is launched).
typedef hipError_t (*LanczosFromYuvLauncher)(const LanczosFromYuvJob &job, hipStream_t stream);

// chipvideo.cpp owns the pointer (null: no kernel unit in this build — the entries answer CHV_ERR_NOT_IMPLEMENTED); the kernel unit
// registers its launcher when the library is loaded.  The host units therefore link without it (tests/stubhip).
void register_lanczos_from_yuv_launcher(LanczosFromYuvLauncher fn);

}  // namespace chv
