// kernels_lanczos_420.hip.cpp — Lanczos-3 between the two 4:2:0 packings (no reference counterpart): the renditions
// of one or several NV12 pictures of one size as y420p pictures of up to eight sizes, or the other way round, every rung in one launch per
// route.  chv_scale_lanczos_420 is the ladder of one rung and one picture.  The construction is lanczos_planar_ladder_body.hip.h's; the row
// code of the chroma planes is lanczos_420_body.hip.h's, luma is planar_strip<T, 1> itself.
//
//   lanczos_420_ladder<MAXT, TO_NV12>   the rungs that take the wave-per-strip route.  A block's work is one strip of one TARGET plane: luma, the
//                                       CbCr plane (TO_NV12: fed from the source's planes 1 AND 2) or one of the two chroma planes (fed from
//                                       component plane - 1 of the source's plane 1).  Two variants by the largest tap class among the launch's
//                                       strip rungs, as in the planar ladder, times the two directions: a kernel holds the bodies of one direction only.
//   lanczos_420_ladder_tile             the rungs that take the tile route, both directions: 256-thread blocks, one per 32 x 4 output bytes.
#include "lanczos_420_body.hip.h"
#include "lanczos_420.h"
#include "lanczos_planar_ladder_body.hip.h"

namespace chv {

struct X420Args {
    const DPlane *batch;              // per picture: n_rungs * n_planes target planes, then the source's planes
    int32_t n_planes, per_image;      // TARGET planes of a picture (2: y420p -> NV12, 3: NV12 -> y420p), planes of a picture's record
    int32_t src_at, rows;             // the source's first plane within a record; output rows per wave (strip route)
    int32_t first[kLanczosPlanarLadderMaxRungs];
    LadderRung420 rung[kLanczosPlanarLadderMaxRungs];
    PlanarPlane pl[kLanczosPlanarLadderMaxRungs * kLanczosPlanarMaxPlanes];
};
static_assert(sizeof(X420Args) <= 4096 - 256, "kernel arguments: 4 KB in all, 256 bytes of them the runtime's");

struct X420Block {                    // (PlanarLadderBlock and src2)
    PlanarPlane g;                    // g.src: the source plane that feeds this target plane (the Cb plane for a CbCr target)
    DPlane src2;                      // the Cr plane of a y420p source when the target plane is CbCr; g.src otherwise
    int T, bx, by, plane;
    bool live;
};

// the source planes of the OTHER packing: luma reads source plane 0, every chroma target plane source plane 1, a CbCr target plane source
// plane 2 as well
template <bool XCD>
CHV_DEV X420Block x420_decode(const X420Args &a, int blk) {
    return planar_ladder_block<XCD, X420Block>(a, blk, [](const X420Args &a, X420Block &o, uint64_t pic) {
        o.g.src = cld<DPlane>(pic + (uint64_t)(a.src_at + (o.plane ? 1 : 0)) * sizeof(DPlane));
        o.src2 = cld<DPlane>(pic + (uint64_t)(a.src_at + (o.plane && a.n_planes == 2 ? 2 : o.plane ? 1 : 0)) * sizeof(DPlane));
    });
}

template <int MAXT, bool TO_NV12>
__global__ __launch_bounds__(64, (MAXT <= 12 ? 5 : 4)) void lanczos_420_ladder(const X420Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t x420_lsm[];
    const X420Block blk = x420_decode<true>(a, blockIdx.x);
    if (!blk.live) return;
    const bool luma = blk.plane == 0;
#define CHV_X4_CASE(TT) case TT: if constexpr (TT <= MAXT) { if (luma) planar_strip<TT, 1>(blk.g, blk.bx, blk.by, a.rows, x420_lsm); \
                                                            else x420_strip<TT, TO_NV12>(blk.g, blk.src2, blk.plane - 1, blk.bx, blk.by, a.rows, x420_lsm); } break
    switch (blk.T) {                  // (uniform)
    CHV_X4_CASE(6); CHV_X4_CASE(8); CHV_X4_CASE(12); CHV_X4_CASE(16); CHV_X4_CASE(22);
    default: break;
    }
#undef CHV_X4_CASE
}

__global__ __launch_bounds__(256) void lanczos_420_ladder_tile(const X420Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t x420_lsm[];
    const X420Block blk = x420_decode<false>(a, blockIdx.x);
    if (!blk.live) return;
    // a chroma plane of a y420p target reads component plane - 1 of the CbCr rows, two bytes a tap; everything else one byte a tap
    const bool split = a.n_planes == 3 && blk.plane > 0;
    x420_tile(blk.g, blk.g.src.ptr + (split ? blk.plane - 1 : 0), blk.g.src.pitch, blk.src2.ptr, blk.src2.pitch, split ? 2 : 1, blk.bx, blk.by, x420_lsm);
}

static hipError_t launch_lanczos_420(const Lanczos420Job &job, hipStream_t stream, int *launches) {
    *launches = 0;
    const int np = job.dst_planes;
    const bool to_nv12 = np == 2;
    if (!((np == 2 && job.src_planes == 3) || (np == 3 && job.src_planes == 2)) || job.n_pictures < 1 || job.n_rungs < 1 ||
        job.n_rungs > kLanczosPlanarLadderMaxRungs || !job.batch)
        return hipErrorInvalidValue;
    X420Args proto{};
    proto.batch = job.batch; proto.n_planes = np; proto.per_image = job.n_rungs * np + job.src_planes; proto.src_at = job.n_rungs * np;
    const auto plane = [&](int r, int p) {
        const Lanczos420Rung &j = job.rung[r];
        return planar_ladder_plane(j.tab[p], DPlane{ nullptr, j.w[p], j.h[p], 0, to_nv12 && p == 1 ? 2 : 1 },
                                   DPlane{ nullptr, p ? job.chroma_w : job.luma_w, p ? job.chroma_h : job.luma_h, 0, !to_nv12 && p ? 2 : 1 });
    };
    PlanarLadderPlan<X420Args> L;
    if (!planar_ladder_plan(&L, proto, job.n_rungs, np, job.n_pictures, plane, x420_strip_route)) return hipErrorInvalidValue;
    return ladder_launch(launches, L.n_strip, [&] {
        if (L.max_t <= 12) {
            if (to_nv12) hipLaunchKernelGGL((lanczos_420_ladder<12, true>), dim3(L.strip_grid), dim3(64), L.strip_lds, stream, L.strip);
            else hipLaunchKernelGGL((lanczos_420_ladder<12, false>), dim3(L.strip_grid), dim3(64), L.strip_lds, stream, L.strip);
        } else {
            if (to_nv12) hipLaunchKernelGGL((lanczos_420_ladder<22, true>), dim3(L.strip_grid), dim3(64), L.strip_lds, stream, L.strip);
            else hipLaunchKernelGGL((lanczos_420_ladder<22, false>), dim3(L.strip_grid), dim3(64), L.strip_lds, stream, L.strip);
        }
    }, L.n_tile, [&] { hipLaunchKernelGGL(lanczos_420_ladder_tile, dim3(L.tile_grid), dim3(256), L.tile_lds, stream, L.tile); });
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct Lanczos420Registrar { Lanczos420Registrar() { register_lanczos_420_launcher(launch_lanczos_420); } } g_lanczos_420_registrar;

}  // namespace chv
