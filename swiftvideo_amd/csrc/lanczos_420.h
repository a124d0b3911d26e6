// lanczos_420.h — what chv_scale_lanczos_420 / chv_scale_lanczos_420_ladder (chipvideo.cpp) and their kernel unit (kernels_lanczos_420.hip.cpp) share.
//
// The cross pairs of the two 4:2:0 packings (NV12 -> y420p, y420p -> NV12): every rung of a ladder — the renditions of
// one or several pictures of one size and one packing as pictures of the OTHER packing of up to CHV_LADDER_MAX_RUNGS sizes — leaves in one
// launch per route.  The bytes are those of chv_scale_lanczos for the same-format pair of the same sizes, logical plane (Y, Cb, Cr) by
// logical plane, stored in the other packing.  Same-format pairs never come here: the entries forward them to the existing launchers.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"
#include "lanczos_planar.h"
#include "lanczos_planar_ladder.h"

namespace chv {

struct Lanczos420Rung {
    // per TARGET plane: the tables of (width of the logical plane in the source, in this rung) and the same for the heights — device memory
    // that stays valid until the launches have run — and the size of the plane in every target of this rung
    LanczosPlaneTables tab[kLanczosPlanarMaxPlanes];
    int32_t w[kLanczosPlanarMaxPlanes], h[kLanczosPlanarMaxPlanes];
};

struct Lanczos420Job {
    int32_t n_rungs;                                   // 1 .. kLanczosPlanarLadderMaxRungs
    Lanczos420Rung rung[kLanczosPlanarLadderMaxRungs];
    int32_t dst_planes, src_planes;                    // (3, 2): NV12 -> y420p; (2, 3): y420p -> NV12
    int32_t chroma_w, luma_w, chroma_h, luma_h;        // the logical planes of every source, in texels (Cb and Cr have one size)
    // The descriptor list: n_pictures pictures of n_rungs * dst_planes + src_planes planes each.  In picture i's record, plane p of rung r's
    // target is at [r * dst_planes + p] and plane p of the source — stored once — at [n_rungs * dst_planes + p].  Memory the device can read
    // that stays unchanged until the launches have run.
    const DPlane *batch;
    int32_t n_pictures;
};

// All launches of one chunk: at most two.  Every rung is checked and every rung's route and launch numbers are computed before the first
// launch: hipErrorInvalidValue for a ladder with a rung that chv_scale_lanczos refuses (nothing is launched).  *launches: the device launches
// made, also when the second of two fails.
typedef hipError_t (*Lanczos420Launcher)(const Lanczos420Job &job, hipStream_t stream, int *launches);

// chipvideo.cpp owns the pointer (null: no kernel unit in this build — the cross pairs answer CHV_ERR_NOT_IMPLEMENTED); the kernel unit
// registers its launcher when the library is loaded.  The host units therefore link without it (tests/stubhip).
void register_lanczos_420_launcher(Lanczos420Launcher fn);

}  // namespace chv
