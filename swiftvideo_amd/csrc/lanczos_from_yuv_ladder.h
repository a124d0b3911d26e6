// lanczos_from_yuv_ladder.h — what chv_scale_lanczos_from_yuv_ladder (chipvideo.cpp) and its kernel unit
// (kernels_lanczos_from_yuv_ladder.hip.cpp) share.
//
// The decoder side's ladder: the renditions of one or several NV12 or y420p pictures of one size as BGRA or RGBA
// planes of up to CHV_LADDER_MAX_RUNGS sizes, every rung in one launch per route.  The bytes are those of chv_scale_lanczos_from_yuv
// (section 4.4.6) for every (rung, picture) pair; only how the work reaches the device is new.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"
#include "lanczos_planar.h"
#include "lanczos_planar_ladder.h"

namespace chv {

struct LanczosFromYuvLadderRung {
    // luma: the tables of (iw, ow) and (ih, oh); chroma: of (cw, ow) and (ch, oh), shared by Cb and Cr — device memory that stays valid
    // until the launches have run
    LanczosPlaneTables luma, chroma;
    int32_t w, h;                                      // the size of every target of this rung
};

struct LanczosFromYuvLadderJob {
    int32_t n_rungs;                                   // 1 .. kLanczosPlanarLadderMaxRungs
    LanczosFromYuvLadderRung rung[kLanczosPlanarLadderMaxRungs];
    int32_t src_planes;                                // 2: NV12, 3: y420p
    int32_t rgba;                                      // the targets' byte order: 0 B, G, R, 255; 1 R, G, B, 255
    int32_t luma_w, luma_h, chroma_w, chroma_h;        // the logical planes of every source, in texels (Cb and Cr have one size)
    int32_t yoff, cy, crv, cgu, cgv, cbu;              // section 4.2's row for the call's colourspace
    // The descriptor list: n_pictures pictures of n_rungs + src_planes planes each.  In picture i's record, rung r's target is at [r] and
    // plane p of the source — stored once — at [n_rungs + p].  Memory the device can read that stays unchanged until the launches have run.
    const DPlane *batch;
    int32_t n_pictures;
};

// All launches of one chunk: at most two.  Every rung is checked and every rung's route and launch numbers are computed before the first
// launch: hipErrorInvalidValue for a ladder with a rung that chv_scale_lanczos_from_yuv refuses (nothing is launched).  *launches: the
// device launches made, also when the second of two fails.
typedef hipError_t (*LanczosFromYuvLadderLauncher)(const LanczosFromYuvLadderJob &job, hipStream_t stream, int *launches);

// chipvideo.cpp owns the pointer (null: no kernel unit in this build — the entry answers CHV_ERR_NOT_IMPLEMENTED); the kernel unit
// registers its launcher when the library is loaded.  The host units therefore link without it (tests/stubhip).
void register_lanczos_from_yuv_ladder_launcher(LanczosFromYuvLadderLauncher fn);

}  // namespace chv
