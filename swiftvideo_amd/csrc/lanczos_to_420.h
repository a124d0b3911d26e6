// lanczos_to_420.h — what chv_scale_lanczos_to_420 / chv_scale_lanczos_to_420_ladder (chipvideo.cpp) and their kernel unit
// (kernels_lanczos_to_420.hip.cpp) share.
//
// The decoder's other five formats (NV21, y422p, y444p, yuvs, zvuy) into the two 4:2:0 packings: every rung of a
// ladder — the renditions of one or several pictures of one size and one format as NV12 or y420p pictures of up to CHV_LADDER_MAX_RUNGS
// sizes — leaves in one launch per route.  The bytes are those of chv_scale_lanczos for a 1-component plane, logical image (Y, Cb, Cr) by
// logical image.  NV12 and y420p sources never come here: the entries forward them to chv_scale_lanczos_420 / _420_ladder.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"
#include "lanczos_planar.h"
#include "lanczos_planar_ladder.h"
#include "lanczos_420.h"

namespace chv {

// how the source's logical images lie in its planes (the values are private to the library)
enum LanczosTo420Source : int32_t {
    kTo420Nv21 = 0,         // 2 planes (1, 2): Y plane 0; Cb byte 1, Cr byte 0 of plane 1's texels
    kTo420Planar = 1,       // 3 planes (1, 1, 1): y422p, y444p — the plane sizes say which
    kTo420Yuvs = 2,         // 1 plane of 2 bytes per pixel: Y0 Cb Y1 Cr
    kTo420Zvuy = 3          // 1 plane of 2 bytes per pixel: Cb Y0 Cr Y1
};

struct LanczosTo420Job {
    int32_t n_rungs;                                   // 1 .. kLanczosPlanarLadderMaxRungs
    // per TARGET plane of a rung: the tables of (size of the logical image in the source, in this rung) and the plane's size (Lanczos420Rung's meaning)
    Lanczos420Rung rung[kLanczosPlanarLadderMaxRungs];
    int32_t source;                                    // LanczosTo420Source
    int32_t dst_planes, src_planes;                    // 2: NV12, 3: y420p; 2, 3 or 1 as the source's kind has them
    int32_t chroma_w, luma_w, chroma_h, luma_h;        // the logical images of every source, in texels (Cb and Cr have one size)
    // The descriptor list: n_pictures pictures of n_rungs * dst_planes + src_planes planes each.  In picture i's record, plane p of rung r's
    // target is at [r * dst_planes + p] and plane p of the source — stored once — at [n_rungs * dst_planes + p].  Memory the device can read
    // that stays unchanged until the launches have run.
    const DPlane *batch;
    int32_t n_pictures;
};

// All launches of one chunk: at most two.  Every rung is checked and every rung's route and launch numbers are computed before the first
// launch: hipErrorInvalidValue for a ladder with a rung in which chv_scale_lanczos refuses any logical image (nothing is launched).
// *launches: the device launches made, also when the second of two fails.
typedef hipError_t (*LanczosTo420Launcher)(const LanczosTo420Job &job, hipStream_t stream, int *launches);

// chipvideo.cpp owns the pointer (null: no kernel unit in this build — the five formats answer CHV_ERR_NOT_IMPLEMENTED, NV12 and y420p sources
// are still forwarded); the kernel unit registers its launcher when the library is loaded.  The host units therefore link without it.
void register_lanczos_to_420_launcher(LanczosTo420Launcher fn);

}  // namespace chv
