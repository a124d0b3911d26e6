// lanczos_to_yuv.h — what chv_scale_lanczos_to_yuv (chipvideo.cpp) and its kernel unit (kernels_lanczos_to_yuv.hip.cpp) share.
//
// One 4-component plane (BGRA or RGBA) is resampled with the Lanczos-3 chain of DESIGN.md section 4.4 and leaves as an NV12 or y420p picture
// through the integer matrix of section 4.5: luma per pixel, chroma from the 2 x 2 box mean of the Lanczos codes (section 4.4.2) — all
// pictures of a batch chunk in ONE launch.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"

namespace chv {

constexpr int kLanczosToYuvMaxPlanes = 3;

struct LanczosToYuvJob {
    // the tables of (source width, target width) and (source height, target height): device memory that stays valid until the launch has run
    const int32_t *fx; const float *wx;
    const int32_t *fy; const float *wy;
    int32_t tx, ty;
    int32_t n_dst;                                     // 2: NV12 (luma, CbCr), 3: y420p (luma, Cb, Cr)
    DPlane dst[kLanczosToYuvMaxPlanes], src;           // picture 0's planes; every picture of a batch has these sizes
    // batch != nullptr: n_pictures pictures, picture i's target planes at batch[i * (n_dst + 1) + p], its source at batch[i * (n_dst + 1) + n_dst],
    // in memory the device can read that stays unchanged until the launch has run.  nullptr: the one picture above travels in the launch's arguments.
    const DPlane *batch;
    int32_t n_pictures;
    // DESIGN.md section 4.5's rows in the source's BYTE order (the host exchanges the first and third column for a BGRA source): the kernels never
    // ask which byte is red
    int32_t yoff, ky[3], ku[3], kv[3];
};

// One launch.  Reports like every launcher, through its return value; hipErrorInvalidValue for a refused reduction (nothing is launched).
typedef hipError_t (*LanczosToYuvLauncher)(const LanczosToYuvJob &job, hipStream_t stream);

// chipvideo.cpp owns the pointer (null: no kernel unit in this build — the entries answer CHV_ERR_NOT_IMPLEMENTED); the kernel unit registers
// its launcher when the library is loaded.  The host units therefore link without it (tests/stubhip).
void register_lanczos_to_yuv_launcher(LanczosToYuvLauncher fn);

}  // namespace chv
