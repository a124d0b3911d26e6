// lanczos_planar_ladder.h — what chv_scale_lanczos_ladder (chipvideo.cpp) and its kernel unit (kernels_lanczos_planar_ladder.hip.cpp) share.
//
// Every rung of a ladder — the renditions of one or several NV12 or y420p pictures of one size as pictures of the same format of up to
// CHV_LADDER_MAX_RUNGS sizes — leaves in one launch per route: the rungs that take the wave-per-strip route in one,
// the rungs that take the tile route in at most one more.  The bytes are those of chv_scale_lanczos, rung by rung, plane by plane.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"
#include "lanczos_planar.h"
#include "lanczos_ladder_grid.h"      // kLanczosPlanarLadderMaxRungs

namespace chv {

struct LanczosPlanarLadderRung {
    // per plane: the tables of (source plane's width, this rung's plane's width) and the same for the heights — device memory that stays
    // valid until the launches have run — and the size of the plane in every target of this rung
    LanczosPlaneTables tab[kLanczosPlanarMaxPlanes];
    int32_t w[kLanczosPlanarMaxPlanes], h[kLanczosPlanarMaxPlanes];
};

struct LanczosPlanarLadderJob {
    int32_t n_rungs;                                   // 1 .. kLanczosPlanarLadderMaxRungs
    LanczosPlanarLadderRung rung[kLanczosPlanarLadderMaxRungs];
    int32_t n_planes;                                  // 2: NV12 (planes of 1 and 2 components), 3: y420p (three planes of 1)
    int32_t src_w[kLanczosPlanarMaxPlanes], src_h[kLanczosPlanarMaxPlanes];      // the planes of every source
    // The descriptor list: n_pictures pictures of (n_rungs + 1) * n_planes planes each.  Picture i's record starts at
    // batch[i * (n_rungs + 1) * n_planes]; in it, plane p of rung r's target is at [r * n_planes + p] and plane p of the source — stored once —
    // at [n_rungs * n_planes + p].  Memory the device can read that stays unchanged until the launches have run.
    const DPlane *batch;
    int32_t n_pictures;
};

// All launches of one chunk: at most two.  Every rung is checked and every rung's route and launch numbers are computed before the first
// launch: hipErrorInvalidValue for a ladder with a rung that chv_scale_lanczos refuses (nothing is launched).  *launches: the device launches
// made, also when the second of two fails.
typedef hipError_t (*LanczosPlanarLadderLauncher)(const LanczosPlanarLadderJob &job, hipStream_t stream, int *launches);

// chipvideo.cpp owns the pointer (null: no kernel unit in this build — the entry answers CHV_ERR_NOT_IMPLEMENTED); the kernel unit registers
// its launcher when the library is loaded.  The host units therefore link without it (tests/stubhip).
void register_lanczos_planar_ladder_launcher(LanczosPlanarLadderLauncher fn);

}  // namespace chv
