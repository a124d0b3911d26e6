// kernels_lanczos_to_420.hip.cpp — Lanczos-3 from the decoder's other five formats into the two 4:2:0 packings (no
// reference counterpart): the renditions of one or several NV21, y422p, y444p, yuvs or zvuy pictures of one size as NV12 or y420p pictures of
// up to eight sizes, every rung in one launch per route.  chv_scale_lanczos_to_420 is the ladder of one rung and one picture.  The
// construction is kernels_lanczos_420.hip.cpp's: one grid, the concatenation of the rungs' block ranges, largest first; a scalar scan finds
// the rung.  A block's work is one strip of one TARGET plane; what differs per (source, target) cell is how a lane finds its source bytes:
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

#include <climits>

namespace chv {

struct To420Rung {
    int32_t first_block;              // where the rung's range starts in the grid
    int32_t total, per_picture;       // blocks of all pictures, blocks per picture
    int32_t T;                        // strip route: the rung's tap class
    int32_t dst_at;                   // the rung's first target plane within a picture's record
    int32_t pad[3];
};

// (the size and the access rules of PlanarLadderArgs: read through the scalar unit at a uniform index, never from a private copy)
struct To420Args {
    const DPlane *batch;              // per picture: n_rungs * n_planes target planes, then the source's planes
    int32_t n_planes, per_image;      // TARGET planes of a picture (2: NV12, 3: y420p), planes of a picture's record
    int32_t src_at, rows;             // the source's first plane within a record; output rows per wave (strip route)
    int32_t source, pad;              // LanczosTo420Source
    int32_t first[kLanczosPlanarLadderMaxRungs];
    To420Rung rung[kLanczosPlanarLadderMaxRungs];
    // rung k's target plane p at [k * kLanczosPlanarMaxPlanes + p]; src: the LOGICAL image that feeds the plane (texels), comps its tap stride
    PlanarPlane pl[kLanczosPlanarLadderMaxRungs * kLanczosPlanarMaxPlanes];
};
static_assert(sizeof(To420Args) <= 4096 - 256, "kernel arguments: 4 KB in all, 256 bytes of them the runtime's");

struct To420Block {
    PlanarPlane g;                    // g.src: the logical image's size with the start and pitch of the plane that holds it
    DPlane src2;                      // the Cr plane of a planar source when the target plane is CbCr; g.src otherwise
    int T, bx, by, plane;
    bool live;
};

// where the logical images lie: bytes of Y, Cb and Cr within a texel of the plane that holds them
CHV_DEV int to420_y_off(int source) { return source == kTo420Zvuy ? 1 : 0; }
CHV_DEV int to420_cb_off(int source) { return source == kTo420Zvuy ? 0 : 1; }                  // (NV21: byte 1 of a CrCb texel)
CHV_DEV int to420_cr_off(int source) { return source == kTo420Yuvs ? 3 : source == kTo420Zvuy ? 2 : 0; }

CHV_DEV int to420_rung_of(const To420Args &a, int b) {
    int r = 0;
#pragma unroll
    for (int k = 1; k < kLanczosPlanarLadderMaxRungs; k++) r = b >= a.first[k] ? k : r;
    return r;
}

// (rung, picture, target plane, row chunk, strip) of block b of the grid — x420_decode with the source plane chosen by the kind of source:
// NV21: luma plane 0, chroma plane 1; planar: target plane p reads source plane p, a CbCr target planes 1 AND 2; packed: everything plane 0.
template <bool XCD>
CHV_DEV To420Block to420_decode(const To420Args &a, int blk) {
    const uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const int r = to420_rung_of(a, blk);
    const To420Rung R = cld<To420Rung>(ka + offsetof(To420Args, rung) + (uint64_t)r * sizeof(To420Rung));
    To420Block o;
    o.T = R.T;
    const int b = blk - R.first_block;
    int idx = b;
    if (XCD) {
        const int per_xcd = (R.total + 7) >> 3;
        idx = (b & 7) * per_xcd + (b >> 3);
        o.live = (b >> 3) < per_xcd && idx < R.total;
    } else {
        o.live = idx < R.total;
    }
    if (!o.live) return o;
    const int picture = idx / R.per_picture, rem = idx - picture * R.per_picture;
    const uint64_t recs = ka + offsetof(To420Args, pl) + (uint64_t)r * kLanczosPlanarMaxPlanes * sizeof(PlanarPlane);
    const int f1 = cld<int32_t>(recs + sizeof(PlanarPlane) + offsetof(PlanarPlane, first));
    const int f2 = cld<int32_t>(recs + 2 * sizeof(PlanarPlane) + offsetof(PlanarPlane, first));
    const int plane = (a.n_planes > 2 && rem >= f2) ? 2 : rem >= f1 ? 1 : 0;
    o.plane = plane;
    o.g = cld<PlanarPlane>(recs + (uint64_t)plane * sizeof(PlanarPlane));
    const int in_plane = rem - o.g.first;
    o.by = in_plane / o.g.strips;
    o.bx = in_plane - o.by * o.g.strips;
    const uint64_t pic = (uint64_t)(uintptr_t)a.batch + (uint64_t)picture * a.per_image * sizeof(DPlane);
    o.g.dst = cld<DPlane>(pic + (uint64_t)(R.dst_at + plane) * sizeof(DPlane));
    const int chroma = plane ? 1 : 0;
    const int pa = a.source == kTo420Nv21 ? chroma : a.source == kTo420Planar ? (a.n_planes == 2 ? chroma : plane) : 0;
    const int pb = a.source == kTo420Planar && a.n_planes == 2 && plane ? 2 : pa;
    const DPlane sa = cld<DPlane>(pic + (uint64_t)(a.src_at + pa) * sizeof(DPlane));
    o.src2 = cld<DPlane>(pic + (uint64_t)(a.src_at + pb) * sizeof(DPlane));
    o.g.src.ptr = sa.ptr; o.g.src.pitch = sa.pitch;                // (w, h: the logical image's, from the launch's record)
    return o;
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

// one rung of one route, before the launch's order is known
struct To420Pending {
    To420Rung R;
    PlanarPlane pl[kLanczosPlanarMaxPlanes];
};

// the records of one launch, largest range first; false when the grid would not fit 30 bits
static bool to420_order(To420Args *a, const To420Pending *rungs, int n, int pad, unsigned *grid) {
    int order[kLanczosPlanarLadderMaxRungs];
    for (int k = 0; k < n; k++) order[k] = k;
    std::stable_sort(order, order + n, [&](int x, int y) { return rungs[x].R.total > rungs[y].R.total; });
    long first = 0;
    for (int k = 0; k < kLanczosPlanarLadderMaxRungs; k++) a->first[k] = INT_MAX;
    for (int k = 0; k < n; k++) {
        a->rung[k] = rungs[order[k]].R;
        for (int p = 0; p < kLanczosPlanarMaxPlanes; p++) a->pl[k * kLanczosPlanarMaxPlanes + p] = rungs[order[k]].pl[p];
        a->rung[k].first_block = (int32_t)first;
        a->first[k] = (int32_t)first;
        first += ((long)a->rung[k].total + pad - 1) / pad * pad;
        if (first > 0x3fffffff) return false;
    }
    *grid = (unsigned)first;
    return true;
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
    // every rung's route and numbers before anything is launched: one refused rung refuses the ladder
    To420Pending strip[kLanczosPlanarLadderMaxRungs], tile[kLanczosPlanarLadderMaxRungs];
    int strip_ring[kLanczosPlanarLadderMaxRungs];
    int n_strip = 0, n_tile = 0, max_t = 0;
    size_t tile_lds = 0;
    long work = 0;
    for (int r = 0; r < job.n_rungs; r++) {
        const Lanczos420Rung &j = job.rung[r];
        To420Pending P{};
        for (int p = 0; p < np; p++) {
            const LanczosPlaneTables &t = j.tab[p];
            PlanarPlane &g = P.pl[p];
            g.fx = t.fx; g.wx = t.wx; g.fy = t.fy; g.wy = t.wy; g.tx = t.tx; g.ty = t.ty;
            g.dst = DPlane{ nullptr, j.w[p], j.h[p], 0, to_nv12 && p == 1 ? 2 : 1 };
            // the tap stride of the logical image that feeds this plane; a CbCr target fed from two planar planes stages one row of each
            const int sc = packed ? (p ? 4 : 2) : job.source == kTo420Nv21 && p ? 2 : 1;
            g.src = DPlane{ nullptr, p ? job.chroma_w : job.luma_w, p ? job.chroma_h : job.luma_h, 0, sc };
            if (g.dst.w < 1 || g.dst.h < 1 || g.src.w < 1 || g.src.h < 1 || planar_refuses(g.dst, g.src, t.tx, t.ty)) return hipErrorInvalidValue;
        }
        P.R.dst_at = r * np;
        int T = 0, ring = 0;
        if (x420_strip_route(P.pl, np, &T, &ring)) {
            P.R.T = T;
            work += planar_strip_work(P.pl, np) * job.n_pictures;
            max_t = std::max(max_t, T);
            strip_ring[n_strip] = ring;
            strip[n_strip++] = P;
        } else {
            int rows_max = 0;
            P.R.per_picture = planar_tile_blocks(P.pl, np, &rows_max);
            const long total = (long)P.R.per_picture * job.n_pictures;
            const size_t lds = (size_t)rows_max * PT_W * sizeof(float);
            if (total > 0x3fffffff || lds > 64 * 1024) return hipErrorInvalidValue;
            P.R.total = (int32_t)total;
            tile_lds = std::max(tile_lds, lds);
            tile[n_tile++] = P;
        }
    }
    const int rows = planar_strip_rows(work);
    size_t strip_lds = 0;
    for (int k = 0; k < n_strip; k++) {
        To420Pending &P = strip[k];
        P.R.per_picture = planar_strip_blocks(P.pl, np, rows);
        const long total = (long)P.R.per_picture * job.n_pictures;
        if (total > 0x3fffffff) return hipErrorInvalidValue;
        P.R.total = (int32_t)total;
        strip_lds = std::max(strip_lds, planar_wtab_bytes(rows, P.R.T) + (size_t)2 * strip_ring[k] * 16);
    }
    To420Args a{};
    a.batch = job.batch; a.n_planes = np; a.per_image = job.n_rungs * np + job.src_planes; a.src_at = job.n_rungs * np; a.rows = rows;
    a.source = job.source;
    To420Args t = a;
    unsigned strip_grid = 0, tile_grid = 0;
    if (n_strip && !to420_order(&a, strip, n_strip, 8, &strip_grid)) return hipErrorInvalidValue;
    if (n_tile && !to420_order(&t, tile, n_tile, 1, &tile_grid)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    if (n_strip) {
        if (job.source == kTo420Nv21) to420_launch_strip<kTo420Nv21>(max_t <= 12, strip_grid, strip_lds, stream, a);
        else if (job.source == kTo420Planar) to420_launch_strip<kTo420Planar>(max_t <= 12, strip_grid, strip_lds, stream, a);
        else to420_launch_strip<kTo420Yuvs>(max_t <= 12, strip_grid, strip_lds, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
    }
    if (n_tile) {
        hipLaunchKernelGGL(lanczos_to_420_ladder_tile, dim3(tile_grid), dim3(256), tile_lds, stream, t);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
    }
    return hipSuccess;
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosTo420Registrar { LanczosTo420Registrar() { register_lanczos_to_420_launcher(launch_lanczos_to_420); } } g_lanczos_to_420_registrar;

}  // namespace chv
