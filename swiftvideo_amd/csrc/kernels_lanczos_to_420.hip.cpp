// kernels_lanczos_to_420.hip.cpp — Lanczos-3 from the decoder's other five formats into the two 4:2:0 packings (no
// reference counterpart): the renditions of one or several NV21, y422p, y444p, yuvs or zvuy pictures of one size as NV12 or y420p pictures of
// up to eight sizes, every rung in one launch per route.  chv_scale_lanczos_to_420 is the ladder of one rung and one picture.  The
// construction is lanczos_planar_ladder_body.hip.h's.  What differs per (source, target) cell is how a lane finds its source bytes:
//
//   source \ target plane   Y                        CbCr of NV12                 Cb, Cr of y420p
//   NV21                    planar_strip<T, 1>       to420_strip<T, 2, 2>         x420_strip<T, false>, component 1 / 0
//   y422p, y444p            planar_strip<T, 1>       x420_strip<T, true>          planar_strip<T, 1>
//   yuvs, zvuy              x420_strip<T, false>     to420_strip<T, 4, 2>         to420_strip<T, 4, 1>
//
//   lanczos_to_420_ladder<MAXT, SRC>   the rungs that take the wave-per-strip route.  SRC: one row of the table (a kernel holds the bodies of one
//                                      kind of source only), times two variants by the largest tap class among the launch's strip rungs.
//   lanczos_to_420_ladder_tile         the rungs that take the tile route, every cell: x420_tile with the cell's start pointers and tap stride.
#include "lanczos_to_420_body.hip.h"
#include "lanczos_to_420.h"
#include "lanczos_planar_ladder_body.hip.h"

namespace chv {

struct To420Args {
    const DPlane *batch;              // per picture: n_rungs * n_planes target planes, then the source's planes
    int32_t n_planes, per_image;      // TARGET planes of a picture (2: NV12, 3: y420p), planes of a picture's record
    int32_t src_at, rows;             // the source's first plane within a record; output rows per wave (strip route)
    int32_t source, pad;              // LanczosTo420Source
    int32_t first[kLanczosPlanarLadderMaxRungs];
    LadderRung420 rung[kLanczosPlanarLadderMaxRungs];
    // pl[].src: the LOGICAL image that feeds the plane (texels), comps its tap stride
    PlanarPlane pl[kLanczosPlanarLadderMaxRungs * kLanczosPlanarMaxPlanes];
};
static_assert(sizeof(To420Args) <= 4096 - 256, "kernel arguments: 4 KB in all, 256 bytes of them the runtime's");

struct To420Block {                   // (PlanarLadderBlock and src2)
    PlanarPlane g;                    // g.src: the logical image's size with the start and pitch of the plane that holds it
    DPlane src2;                      // the Cr plane of a planar source when the target plane is CbCr; g.src otherwise
    int T, bx, by, plane;
    bool live;
};

// where the logical images lie: bytes of Y, Cb and Cr within a texel of the plane that holds them
CHV_DEV int to420_y_off(int source) { return source == kTo420Zvuy ? 1 : 0; }
CHV_DEV int to420_cb_off(int source) { return source == kTo420Zvuy ? 0 : 1; }                  // (NV21: byte 1 of a CrCb texel)
CHV_DEV int to420_cr_off(int source) { return source == kTo420Yuvs ? 3 : source == kTo420Zvuy ? 2 : 0; }

// the source plane by the kind of source — NV21: luma plane 0, chroma plane 1; planar: target plane p reads source plane p, a CbCr target
// planes 1 AND 2; packed: everything plane 0
template <bool XCD>
CHV_DEV To420Block to420_decode(const To420Args &a, int blk) {
    return planar_ladder_block<XCD, To420Block>(a, blk, [](const To420Args &a, To420Block &o, uint64_t pic) {
        const int plane = o.plane, chroma = plane ? 1 : 0;
        const int pa = a.source == kTo420Nv21 ? chroma : a.source == kTo420Planar ? (a.n_planes == 2 ? chroma : plane) : 0;
        const int pb = a.source == kTo420Planar && a.n_planes == 2 && plane ? 2 : pa;
        const DPlane sa = cld<DPlane>(pic + (uint64_t)(a.src_at + pa) * sizeof(DPlane));
        o.src2 = cld<DPlane>(pic + (uint64_t)(a.src_at + pb) * sizeof(DPlane));
        o.g.src.ptr = sa.ptr; o.g.src.pitch = sa.pitch;            // (w, h: the logical image's, from the launch's record)
    });
}

template <int T, int SRC>
CHV_DEV void to420_cell(const To420Args &a, const To420Block &blk, uint8_t *lsm) {
    const bool luma = blk.plane == 0, nv12 = a.n_planes == 2;     // (uniform)
    if constexpr (SRC == kTo420Nv21) {
        if (luma) planar_strip<T, 1>(blk.g, blk.bx, blk.by, a.rows, lsm);
        else if (nv12) to420_strip<T, 2, 2>(blk.g, 1, 0, blk.bx, blk.by, a.rows, lsm);
        else x420_strip<T, false>(blk.g, blk.src2, 2 - blk.plane, blk.bx, blk.by, a.rows, lsm);
    } else if constexpr (SRC == kTo420Planar) {
        if (luma || !nv12) planar_strip<T, 1>(blk.g, blk.bx, blk.by, a.rows, lsm);
        else x420_strip<T, true>(blk.g, blk.src2, 0, blk.bx, blk.by, a.rows, lsm);
    } else {
        const int cb = to420_cb_off(a.source), cr = to420_cr_off(a.source);
        if (luma) x420_strip<T, false>(blk.g, blk.src2, to420_y_off(a.source), blk.bx, blk.by, a.rows, lsm);
        else if (nv12) to420_strip<T, 4, 2>(blk.g, cb, cr, blk.bx, blk.by, a.rows, lsm);
        else to420_strip<T, 4, 1>(blk.g, blk.plane == 1 ? cb : cr, 0, blk.bx, blk.by, a.rows, lsm);
    }
}

// SRC: kTo420Nv21, kTo420Planar, or kTo420Yuvs for both packed orders (a.source tells them apart)
template <int MAXT, int SRC>
__global__ __launch_bounds__(64, (MAXT <= 12 ? 5 : 4)) void lanczos_to_420_ladder(const To420Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t to420_lsm[];
    const To420Block blk = to420_decode<true>(a, blockIdx.x);
    if (!blk.live) return;
#define CHV_T4_CASE(TT) case TT: if constexpr (TT <= MAXT) to420_cell<TT, SRC>(a, blk, to420_lsm); break
    switch (blk.T) {                  // (uniform)
    CHV_T4_CASE(6); CHV_T4_CASE(8); CHV_T4_CASE(12); CHV_T4_CASE(16); CHV_T4_CASE(22);
    default: break;
    }
#undef CHV_T4_CASE
}

__global__ __launch_bounds__(256) void lanczos_to_420_ladder_tile(const To420Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t to420_lsm[];
    const To420Block blk = to420_decode<false>(a, blockIdx.x);
    if (!blk.live) return;
    const bool luma = blk.plane == 0, nv12 = a.n_planes == 2;
    // the start of component 0's (or the only component's) taps, of component 1's, and the bytes between two taps
    int oa = 0, ob = 0, stride = 1;
    if (a.source == kTo420Nv21) {
        if (!luma) { stride = 2; oa = nv12 ? 1 : 2 - blk.plane; }
    } else if (a.source != kTo420Planar) {
        const int cb = to420_cb_off(a.source), cr = to420_cr_off(a.source);
        stride = luma ? 2 : 4;
        oa = luma ? to420_y_off(a.source) : nv12 || blk.plane == 1 ? cb : cr;
        ob = cr;
    }
    x420_tile(blk.g, blk.g.src.ptr + oa, blk.g.src.pitch, blk.src2.ptr + ob, blk.src2.pitch, stride, blk.bx, blk.by, to420_lsm);
}

template <int SRC>
static void to420_launch_strip(bool small, unsigned grid, size_t lds, hipStream_t stream, const To420Args &a) {
    if (small) hipLaunchKernelGGL((lanczos_to_420_ladder<12, SRC>), dim3(grid), dim3(64), lds, stream, a);
    else hipLaunchKernelGGL((lanczos_to_420_ladder<22, SRC>), dim3(grid), dim3(64), lds, stream, a);
}

static hipError_t launch_lanczos_to_420(const LanczosTo420Job &job, hipStream_t stream, int *launches) {
    *launches = 0;
    const int np = job.dst_planes;
    const bool to_nv12 = np == 2;
    const int want_src = job.source == kTo420Nv21 ? 2 : job.source == kTo420Planar ? 3 : 1;
    if ((np != 2 && np != 3) || job.source < kTo420Nv21 || job.source > kTo420Zvuy || job.src_planes != want_src || job.n_pictures < 1 ||
        job.n_rungs < 1 || job.n_rungs > kLanczosPlanarLadderMaxRungs || !job.batch)
        return hipErrorInvalidValue;
    const bool packed = job.source == kTo420Yuvs || job.source == kTo420Zvuy;
    To420Args proto{};
    proto.batch = job.batch; proto.n_planes = np; proto.per_image = job.n_rungs * np + job.src_planes; proto.src_at = job.n_rungs * np;
    proto.source = job.source;
    const auto plane = [&](int r, int p) {
        const Lanczos420Rung &j = job.rung[r];
        // the tap stride of the logical image that feeds this plane; a CbCr target fed from two planar planes stages one row of each
        const int sc = packed ? (p ? 4 : 2) : job.source == kTo420Nv21 && p ? 2 : 1;
        return planar_ladder_plane(j.tab[p], DPlane{ nullptr, j.w[p], j.h[p], 0, to_nv12 && p == 1 ? 2 : 1 },
                                   DPlane{ nullptr, p ? job.chroma_w : job.luma_w, p ? job.chroma_h : job.luma_h, 0, sc });
    };
    PlanarLadderPlan<To420Args> L;
    if (!planar_ladder_plan(&L, proto, job.n_rungs, np, job.n_pictures, plane, x420_strip_route)) return hipErrorInvalidValue;
    return ladder_launch(launches, L.n_strip, [&] {
        if (job.source == kTo420Nv21) to420_launch_strip<kTo420Nv21>(L.max_t <= 12, L.strip_grid, L.strip_lds, stream, L.strip);
        else if (job.source == kTo420Planar) to420_launch_strip<kTo420Planar>(L.max_t <= 12, L.strip_grid, L.strip_lds, stream, L.strip);
        else to420_launch_strip<kTo420Yuvs>(L.max_t <= 12, L.strip_grid, L.strip_lds, stream, L.strip);
    }, L.n_tile, [&] { hipLaunchKernelGGL(lanczos_to_420_ladder_tile, dim3(L.tile_grid), dim3(256), L.tile_lds, stream, L.tile); });
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosTo420Registrar { LanczosTo420Registrar() { register_lanczos_to_420_launcher(launch_lanczos_to_420); } } g_lanczos_to_420_registrar;

}  // namespace chv
