// lanczos_ladder.h — what chv_scale_lanczos_to_yuv_ladder (chipvideo.cpp) and its kernel unit (kernels_lanczos_ladder.hip.cpp) share.
//
// Every rung of a ladder — the renditions of one or several BGRA / RGBA canvases of one size as NV12 or y420p pictures of up to
// CHV_LADDER_MAX_RUNGS sizes — leaves in one launch per route: the rungs that take the wave-per-strip route in one,
// the rungs that take the tile route in at most one more.  The bytes are those of chv_scale_lanczos_to_yuv, rung by rung.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"

namespace chv {

constexpr int kLanczosLadderMaxRungs = 8;

struct LanczosLadderRung {
    // the tables of (source width, this rung's width) and (source height, this rung's height): device memory that stays valid until the
    // launches have run
    const int32_t *fx; const float *wx;
    const int32_t *fy; const float *wy;
    int32_t tx, ty;
    int32_t w, h;                                      // plane 0 of every target of this rung
};

struct LanczosLadderJob {
    int32_t n_rungs;                                   // 1 .. kLanczosLadderMaxRungs
    LanczosLadderRung rung[kLanczosLadderMaxRungs];
    int32_t src_w, src_h;                              // every source
    int32_t n_dst;                                     // 2: NV12 (luma, CbCr), 3: y420p (luma, Cb, Cr)
    // n_pictures pictures of n_rungs * n_dst + 1 planes each: rung r's target planes of picture i at batch[i * (n_rungs * n_dst + 1) + r * n_dst + p],
    // its source at batch[i * (n_rungs * n_dst + 1) + n_rungs * n_dst] — in memory the device can read that stays unchanged until the launches have run
    const DPlane *batch;
    int32_t n_pictures;
    // DESIGN.md section 4.5's rows in the source's BYTE order, as in LanczosToYuvJob
    int32_t yoff, ky[3], ku[3], kv[3];
};

// All launches of one chunk: at most two.  Every rung is checked before the first launch: hipErrorInvalidValue for a ladder with a rung that
// chv_scale_lanczos_to_yuv refuses (nothing is launched).  *launches: the device launches made, also when the second of two fails.
typedef hipError_t (*LanczosLadderLauncher)(const LanczosLadderJob &job, hipStream_t stream, int *launches);

// chipvideo.cpp owns the pointer (null: no kernel unit in this build — the entry answers CHV_ERR_NOT_IMPLEMENTED); the kernel unit registers
// its launcher when the library is loaded.  The host units therefore link without it (tests/stubhip).
void register_lanczos_ladder_launcher(LanczosLadderLauncher fn);

}  // namespace chv
