// lanczos_hbd.h — what chv_scale_lanczos_hbd_to_420 / chv_scale_lanczos_hbd_to_420_ladder (chipvideo.cpp) and their kernel unit
// (kernels_lanczos_hbd.hip.cpp) share.
//
// The two 10-bit 4:2:0 formats (P010, yuv420p10le) into the two 8-bit 4:2:0 packings: every rung of a ladder — the
// renditions of one or several pictures of one size and one format as NV12 or y420p pictures of up to CHV_LADDER_MAX_RUNGS sizes — leaves
// in one launch per route.  Y, Cb and Cr are each resampled as chv_scale_lanczos resamples a 1-component plane, on the 10-bit codes, and the
// value that leaves the vertical chain is stored as convert_uchar_sat_rte(v * 0.25f).  No 8-bit source comes here.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"
#include "lanczos_planar.h"
#include "lanczos_planar_ladder.h"
#include "lanczos_420.h"
#include "lanczos_route.h"

namespace chv {

// how the source's logical images lie in its planes (the values are private to the library)
enum LanczosHbdSource : int32_t {
    kHbdP010 = 0,           // 2 planes of 2 and 4 bytes per texel: Y; Cb word 0, Cr word 1.  The code is word >> 6
    kHbdPlanar = 1          // 3 planes of 2 bytes per texel: Y, Cb, Cr (yuv420p10le).  The code is word & 1023
};

struct LanczosHbdJob {
    int32_t n_rungs;                                   // 1 .. kLanczosPlanarLadderMaxRungs
    // per TARGET plane of a rung: the tables of (size of the logical image in the source, in this rung) and the plane's size (Lanczos420Rung's meaning)
    Lanczos420Rung rung[kLanczosPlanarLadderMaxRungs];
    int32_t source;                                    // LanczosHbdSource
    int32_t dst_planes, src_planes;                    // 2: NV12, 3: y420p; 2: P010, 3: y420p10
    int32_t chroma_w, luma_w, chroma_h, luma_h;        // the logical images of every source, in samples (Cb and Cr have one size)
    // The descriptor list: n_pictures pictures of n_rungs * dst_planes + src_planes planes each.  In picture i's record, plane p of rung r's
    // target is at [r * dst_planes + p] and plane p of the source — stored once — at [n_rungs * dst_planes + p].  Memory the device can read
    // that stays unchanged until the launches have run.
    const DPlane *batch;
    int32_t n_pictures;
};

// the tap stride in bytes of the logical image that feeds target plane p (0: luma): what x420_strip_route takes for src.comps
inline int hbd_tap_stride(int source, int p) { return source == kHbdP010 && p ? 4 : 2; }

// THE routing rule of these entries: x420_strip_route on the geometry with the tap strides above.  A CbCr target fed from the two chroma
// planes of y420p10 stages one row of EACH in a ring slot: *ring_max counts both (2 nv <= 40 for every strip-route geometry, so the route
// is x420_strip_route's own answer).
inline bool hbd_strip_route_p010(PlanarPlane *pl, int np, int *T, int *ring_max) { return x420_strip_route(pl, np, T, ring_max); }
inline bool hbd_strip_route_planar(PlanarPlane *pl, int np, int *T, int *ring_max) {
    const bool strip = x420_strip_route(pl, np, T, ring_max);
    for (int p = 0; p < np; p++)
        if (pl[p].dst.comps == 2) *ring_max = std::max(*ring_max, 2 * pl[p].nv);
    return strip && *ring_max <= 64;
}

// All launches of one chunk: at most two.  Every rung is checked and every rung's route and launch numbers are computed before the first
// launch: hipErrorInvalidValue for a ladder with a rung in which chv_scale_lanczos refuses any logical image (nothing is launched).
// *launches: the device launches made, also when the second of two fails.
typedef hipError_t (*LanczosHbdLauncher)(const LanczosHbdJob &job, hipStream_t stream, int *launches);

// chipvideo.cpp owns the pointer (null: no kernel unit in this build — the entries answer CHV_ERR_NOT_IMPLEMENTED after validation); the
// kernel unit registers its launcher when the library is loaded.  The host units therefore link without it (tests/stubhip).
void register_lanczos_hbd_launcher(LanczosHbdLauncher fn);

}  // namespace chv
