// lanczos_rgb_ladder.h — what chv_scale_lanczos_rgb_ladder (chipvideo.cpp) and its kernel unit (kernels_lanczos_rgb_ladder.hip.cpp) share.
//
// The ladder of 4-component planes: the renditions of one or several BGRA or RGBA planes of one size as planes of
// the same byte order of up to CHV_LADDER_MAX_RUNGS sizes, every rung in one launch per route.  The bytes are those of chv_scale_lanczos
// on one 4-component plane (section 4.4) for every (rung, picture) pair; only how the work reaches the device is new.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"
#include "lanczos_planar.h"
#include "lanczos_planar_ladder.h"

namespace chv {

struct LanczosRgbLadderRung {
    // the tables of (src_w, w) and (src_h, h): device memory that stays valid until the launches have run
    LanczosPlaneTables tab;
    int32_t w, h;                                      // the size of every target of this rung
};

struct LanczosRgbLadderJob {
    int32_t n_rungs;                                   // 1 .. kLanczosPlanarLadderMaxRungs
    LanczosRgbLadderRung rung[kLanczosPlanarLadderMaxRungs];
    int32_t src_w, src_h;                              // the size of every source, in texels
    // The descriptor list: n_pictures pictures of n_rungs + 1 planes each.  In picture i's record, rung r's target is at [r] and the
    // source — stored once — at [n_rungs].  Memory the device can read that stays unchanged until the launches have run.
    const DPlane *batch;
    int32_t n_pictures;
};

// All launches of one chunk: at most two.  Every rung is checked and every rung's route and launch numbers are computed before the first
// launch: hipErrorInvalidValue for a ladder with a rung that chv_scale_lanczos refuses (nothing is launched).  *launches: the device
// launches made, also when the second of two fails.
typedef hipError_t (*LanczosRgbLadderLauncher)(const LanczosRgbLadderJob &job, hipStream_t stream, int *launches);

// chipvideo.cpp owns the pointer (null: no kernel unit in this build — the entry answers CHV_ERR_NOT_IMPLEMENTED); the kernel unit
// registers its launcher when the library is loaded.  The host units therefore link without it (tests/stubhip).
void register_lanczos_rgb_ladder_launcher(LanczosRgbLadderLauncher fn);

}  // namespace chv
