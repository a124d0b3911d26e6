// kernels_lanczos_420.hip.cpp — Lanczos-3 between the two 4:2:0 packings (no reference counterpart): the renditions
// of one or several NV12 pictures of one size as y420p pictures of up to eight sizes, or the other way round, every rung in one launch per
// route.  chv_scale_lanczos_420 is the ladder of one rung and one picture.  The construction is kernels_lanczos_planar_ladder.hip.cpp's: one
// grid, the concatenation of the rungs' block ranges, largest first; a scalar scan finds the rung.  The row code of the chroma planes is
// lanczos_420_body.hip.h's, luma is planar_strip<T, 1> itself.
//
//   lanczos_420_ladder<MAXT, TO_NV12>   the rungs that take the wave-per-strip route.  A block's work is one strip of one TARGET plane: luma, the
//                                       CbCr plane (TO_NV12: fed from the source's planes 1 AND 2) or one of the two chroma planes (fed from
//                                       component plane - 1 of the source's plane 1).  Two variants by the largest tap class among the launch's
//                                       strip rungs, as in the planar ladder, times the two directions: a kernel holds the bodies of one direction only.
//   lanczos_420_ladder_tile             the rungs that take the tile route, both directions: 256-thread blocks, one per 32 x 4 output bytes.
#include "lanczos_420_body.hip.h"
#include "lanczos_420.h"

#include <climits>

namespace chv {

struct X420Rung {
    int32_t first_block;              // where the rung's range starts in the grid
    int32_t total, per_picture;       // blocks of all pictures, blocks per picture
    int32_t T;                        // strip route: the rung's tap class
    int32_t dst_at;                   // the rung's first target plane within a picture's record
    int32_t pad[3];
};

// (the size and the access rules of PlanarLadderArgs: read through the scalar unit at a uniform index, never from a private copy)
struct X420Args {
    const DPlane *batch;              // per picture: n_rungs * n_planes target planes, then the source's planes
    int32_t n_planes, per_image;      // TARGET planes of a picture (2: y420p -> NV12, 3: NV12 -> y420p), planes of a picture's record
    int32_t src_at, rows;             // the source's first plane within a record; output rows per wave (strip route)
    int32_t first[kLanczosPlanarLadderMaxRungs];
    X420Rung rung[kLanczosPlanarLadderMaxRungs];
    PlanarPlane pl[kLanczosPlanarLadderMaxRungs * kLanczosPlanarMaxPlanes];      // rung k's target plane p at [k * kLanczosPlanarMaxPlanes + p]
};
static_assert(sizeof(X420Args) <= 4096 - 256, "kernel arguments: 4 KB in all, 256 bytes of them the runtime's");

struct X420Block {
    PlanarPlane g;                    // g.src: the source plane that feeds this target plane (the Cb plane for a CbCr target)
    DPlane src2;                      // the Cr plane of a y420p source when the target plane is CbCr; g.src otherwise
    int T, bx, by, plane;
    bool live;
};

CHV_DEV int x420_rung_of(const X420Args &a, int b) {
    int r = 0;
#pragma unroll
    for (int k = 1; k < kLanczosPlanarLadderMaxRungs; k++) r = b >= a.first[k] ? k : r;
    return r;
}

// (rung, picture, target plane, row chunk, strip) of block b of the grid — planar_ladder_decode with the source planes of the OTHER packing:
// luma reads source plane 0, every chroma target plane source plane 1, a CbCr target plane source plane 2 as well.
template <bool XCD>
CHV_DEV X420Block x420_decode(const X420Args &a, int blk) {
    const uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const int r = x420_rung_of(a, blk);
    const X420Rung R = cld<X420Rung>(ka + offsetof(X420Args, rung) + (uint64_t)r * sizeof(X420Rung));
    X420Block o;
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
    const uint64_t recs = ka + offsetof(X420Args, pl) + (uint64_t)r * kLanczosPlanarMaxPlanes * sizeof(PlanarPlane);
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
    o.g.src = cld<DPlane>(pic + (uint64_t)(a.src_at + (plane ? 1 : 0)) * sizeof(DPlane));
    o.src2 = cld<DPlane>(pic + (uint64_t)(a.src_at + (plane && a.n_planes == 2 ? 2 : plane ? 1 : 0)) * sizeof(DPlane));
    return o;
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

// one rung of one route, before the launch's order is known
struct X420Pending {
    X420Rung R;
    PlanarPlane pl[kLanczosPlanarMaxPlanes];
};

// the records of one launch, largest range first; false when the grid would not fit 30 bits
static bool x420_order(X420Args *a, const X420Pending *rungs, int n, int pad, unsigned *grid) {
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

static hipError_t launch_lanczos_420(const Lanczos420Job &job, hipStream_t stream, int *launches) {
    *launches = 0;
    const int np = job.dst_planes;
    const bool to_nv12 = np == 2;
    if (!((np == 2 && job.src_planes == 3) || (np == 3 && job.src_planes == 2)) || job.n_pictures < 1 || job.n_rungs < 1 ||
        job.n_rungs > kLanczosPlanarLadderMaxRungs || !job.batch)
        return hipErrorInvalidValue;
    // every rung's route and numbers before anything is launched: one refused rung refuses the ladder
    X420Pending strip[kLanczosPlanarLadderMaxRungs], tile[kLanczosPlanarLadderMaxRungs];
    int strip_ring[kLanczosPlanarLadderMaxRungs];
    int n_strip = 0, n_tile = 0, max_t = 0;
    size_t tile_lds = 0;
    long work = 0;
    for (int r = 0; r < job.n_rungs; r++) {
        const Lanczos420Rung &j = job.rung[r];
        X420Pending P{};
        for (int p = 0; p < np; p++) {
            const LanczosPlaneTables &t = j.tab[p];
            PlanarPlane &g = P.pl[p];
            g.fx = t.fx; g.wx = t.wx; g.fy = t.fy; g.wy = t.wy; g.tx = t.tx; g.ty = t.ty;
            g.dst = DPlane{ nullptr, j.w[p], j.h[p], 0, to_nv12 && p == 1 ? 2 : 1 };
            g.src = DPlane{ nullptr, p ? job.chroma_w : job.luma_w, p ? job.chroma_h : job.luma_h, 0, !to_nv12 && p ? 2 : 1 };
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
        X420Pending &P = strip[k];
        P.R.per_picture = planar_strip_blocks(P.pl, np, rows);
        const long total = (long)P.R.per_picture * job.n_pictures;
        if (total > 0x3fffffff) return hipErrorInvalidValue;
        P.R.total = (int32_t)total;
        strip_lds = std::max(strip_lds, planar_wtab_bytes(rows, P.R.T) + (size_t)2 * strip_ring[k] * 16);
    }
    X420Args a{};
    a.batch = job.batch; a.n_planes = np; a.per_image = job.n_rungs * np + job.src_planes; a.src_at = job.n_rungs * np; a.rows = rows;
    X420Args t = a;
    unsigned strip_grid = 0, tile_grid = 0;
    if (n_strip && !x420_order(&a, strip, n_strip, 8, &strip_grid)) return hipErrorInvalidValue;
    if (n_tile && !x420_order(&t, tile, n_tile, 1, &tile_grid)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    if (n_strip) {
        if (max_t <= 12) {
            if (to_nv12) hipLaunchKernelGGL((lanczos_420_ladder<12, true>), dim3(strip_grid), dim3(64), strip_lds, stream, a);
            else hipLaunchKernelGGL((lanczos_420_ladder<12, false>), dim3(strip_grid), dim3(64), strip_lds, stream, a);
        } else {
            if (to_nv12) hipLaunchKernelGGL((lanczos_420_ladder<22, true>), dim3(strip_grid), dim3(64), strip_lds, stream, a);
            else hipLaunchKernelGGL((lanczos_420_ladder<22, false>), dim3(strip_grid), dim3(64), strip_lds, stream, a);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
    }
    if (n_tile) {
        hipLaunchKernelGGL(lanczos_420_ladder_tile, dim3(tile_grid), dim3(256), tile_lds, stream, t);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
    }
    return hipSuccess;
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct Lanczos420Registrar { Lanczos420Registrar() { register_lanczos_420_launcher(launch_lanczos_420); } } g_lanczos_420_registrar;

}  // namespace chv
