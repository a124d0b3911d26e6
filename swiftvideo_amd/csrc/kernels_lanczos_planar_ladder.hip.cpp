// kernels_lanczos_planar_ladder.hip.cpp — every rung of a 4:2:0 encoder ladder in one launch per route (no reference
// counterpart): the renditions of one or several NV12 or y420p pictures of one size as pictures of the same format of up to eight sizes.  The
// row code is that of chv_scale_lanczos on such pictures (lanczos_planar_body.hip.h), so the bytes are; how a block finds its work and how
// the launches are planned is lanczos_planar_ladder_body.hip.h's.
//
//   planar_lanczos_ladder<MAXT>   the rungs that take the wave-per-strip route: dispatches (uniformly) on the rung's tap class and the plane's
//                                 components to the shared strip body.  A kernel is allocated the registers of its largest body, hence two
//                                 variants by the largest tap class among the launch's strip rungs: <12> holds the bodies of 6, 8 and 12
//                                 taps at five waves per SIMD, <22> all five at four.
//   planar_lanczos_ladder_tile    the rungs that take the tile route, over the shared tile body: 256-thread blocks, one per 32 x 4 output bytes.
#include "lanczos_planar_ladder_body.hip.h"

namespace chv {

struct PlanarLadderArgs {
    const DPlane *batch;              // per picture: n_rungs * n_planes target planes, then the n_planes source planes
    int32_t n_planes, per_image;      // planes of a picture, planes of a picture's record
    int32_t src_at, rows;             // the source's first plane within a record; output rows per wave (strip route: one count for the launch)
    int32_t first[kLanczosPlanarLadderMaxRungs];       // first_block of rung k of this launch (INT_MAX beyond the last): what the scan reads
    LadderRung420 rung[kLanczosPlanarLadderMaxRungs];
    PlanarPlane pl[kLanczosPlanarLadderMaxRungs * kLanczosPlanarMaxPlanes];
};
static_assert(sizeof(PlanarLadderArgs) <= 4096 - 256, "kernel arguments: 4 KB in all, 256 bytes of them the runtime's");

// target plane p reads source plane p
template <bool XCD>
CHV_DEV PlanarLadderBlock planar_ladder_decode(const PlanarLadderArgs &a, int blk) {
    return planar_ladder_block<XCD, PlanarLadderBlock>(a, blk, [](const PlanarLadderArgs &a, PlanarLadderBlock &o, uint64_t pic) {
        o.g.src = cld<DPlane>(pic + (uint64_t)(a.src_at + o.plane) * sizeof(DPlane));
    });
}

// <12>: the single kernels of 6, 8 and 12 taps run five waves per SIMD, <22>'s four.  (Should the ladder's decode ever push <12> past 96
// registers, it gets four waves rather than spills: tests/test_lanczos_planar_ladder_contract.py pins what the build gave.)
template <int MAXT>
__global__ __launch_bounds__(64, (MAXT <= 12 ? 5 : 4)) void planar_lanczos_ladder(const PlanarLadderArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t planar_ladder_lsm[];
    const PlanarLadderBlock blk = planar_ladder_decode<true>(a, blockIdx.x);
    if (!blk.live) return;
    const bool two = blk.g.dst.comps == 2;
#define CHV_PL_CASE(TT) case TT: if constexpr (TT <= MAXT) { if (two) planar_strip<TT, 2>(blk.g, blk.bx, blk.by, a.rows, planar_ladder_lsm); \
                                                            else planar_strip<TT, 1>(blk.g, blk.bx, blk.by, a.rows, planar_ladder_lsm); } break
    switch (blk.T) {                  // (uniform)
    CHV_PL_CASE(6); CHV_PL_CASE(8); CHV_PL_CASE(12); CHV_PL_CASE(16); CHV_PL_CASE(22);
    default: break;
    }
#undef CHV_PL_CASE
}

__global__ __launch_bounds__(256) void planar_lanczos_ladder_tile(const PlanarLadderArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t planar_ladder_lsm[];
    const PlanarLadderBlock blk = planar_ladder_decode<false>(a, blockIdx.x);
    if (!blk.live) return;
    planar_tile(blk.g, blk.bx, blk.by, planar_ladder_lsm);
}

static hipError_t launch_lanczos_planar_ladder(const LanczosPlanarLadderJob &job, hipStream_t stream, int *launches) {
    *launches = 0;
    const int np = job.n_planes;
    if ((np != 2 && np != 3) || job.n_pictures < 1 || job.n_rungs < 1 || job.n_rungs > kLanczosPlanarLadderMaxRungs || !job.batch) return hipErrorInvalidValue;
    PlanarLadderArgs proto{};
    proto.batch = job.batch; proto.n_planes = np; proto.per_image = (job.n_rungs + 1) * np; proto.src_at = job.n_rungs * np;
    const auto plane = [&](int r, int p) {
        const LanczosPlanarLadderRung &j = job.rung[r];
        const int comps = np == 2 && p == 1 ? 2 : 1;
        return planar_ladder_plane(j.tab[p], DPlane{ nullptr, j.w[p], j.h[p], 0, comps }, DPlane{ nullptr, job.src_w[p], job.src_h[p], 0, comps });
    };
    PlanarLadderPlan<PlanarLadderArgs> L;
    if (!planar_ladder_plan(&L, proto, job.n_rungs, np, job.n_pictures, plane, planar_strip_route)) return hipErrorInvalidValue;
    return ladder_launch(launches, L.n_strip, [&] {
        if (L.max_t <= 12) hipLaunchKernelGGL(planar_lanczos_ladder<12>, dim3(L.strip_grid), dim3(64), L.strip_lds, stream, L.strip);
        else hipLaunchKernelGGL(planar_lanczos_ladder<22>, dim3(L.strip_grid), dim3(64), L.strip_lds, stream, L.strip);
    }, L.n_tile, [&] { hipLaunchKernelGGL(planar_lanczos_ladder_tile, dim3(L.tile_grid), dim3(256), L.tile_lds, stream, L.tile); });
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosPlanarLadderRegistrar { LanczosPlanarLadderRegistrar() { register_lanczos_planar_ladder_launcher(launch_lanczos_planar_ladder); } } g_lanczos_planar_ladder_registrar;

}  // namespace chv
