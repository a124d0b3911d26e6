// kernels_lanczos_planar_ladder.hip.cpp — every rung of a 4:2:0 encoder ladder in one launch (no reference
// counterpart): the renditions of one or several NV12 or y420p pictures of one size as pictures of the same format of up to eight sizes.  The
// row code is that of chv_scale_lanczos on such pictures (lanczos_planar_body.hip.h), so the bytes are; what is new is how a block finds its work.
//
//   planar_lanczos_ladder<MAXT>   the rungs that take the wave-per-strip route.  ONE grid of 64-thread blocks, the concatenation of the rungs'
//                                 block ranges, largest rung first (the grid's tail is made of the small rungs' blocks).  A block finds its rung
//                                 by a scalar scan of the cumulative block counts in the arguments, then its picture, plane, row chunk and strip
//                                 as planar_lanczos_strip<T> does — with the XCD-aware numbering run PER RUNG: every range starts on a multiple
//                                 of 8 and is padded to one — reads its planes from the descriptor list through the scalar unit, and dispatches
//                                 (uniformly) on the rung's tap class and the plane's components to the shared strip body.  A kernel is
//                                 allocated the registers of its largest body, hence two variants by the largest tap class among the launch's
//                                 strip rungs: <12> holds the bodies of 6, 8 and 12 taps at five waves per SIMD, <22> all five at four.
//   planar_lanczos_ladder_tile    the rungs that take the tile route, the same construction over the shared tile body: 256-thread blocks, one
//                                 per 32 x 4 output bytes.
//
// Dynamic LDS is the maximum over the launch's rungs; the strip body finds its staging ring behind a weight table of ITS OWN tap class.
#include "lanczos_planar_body.hip.h"
#include "lanczos_planar_ladder.h"

#include <climits>

namespace chv {

struct PlanarLadderRung {
    int32_t first_block;              // where the rung's range starts in the grid
    int32_t total, per_picture;       // blocks of all pictures (the range in the grid: `total` rounded up to 8 for strips), blocks per picture
    int32_t T;                        // strip route: the rung's tap class (6 / 8 / 12 / 16 / 22 over its largest tap count)
    int32_t dst_at;                   // the rung's first target plane within a picture's record
    int32_t pad[3];
};

// Up to 8 rungs x 3 planes of records: more than the 1 KB the sibling units allow themselves, inside the 4 KB a launch may carry (the runtime's
// own hidden arguments take 256 bytes of those).  The records are read through the scalar unit at a uniform index, never from a private copy.
struct PlanarLadderArgs {
    const DPlane *batch;              // per picture: n_rungs * n_planes target planes, then the n_planes source planes
    int32_t n_planes, per_image;      // planes of a picture, planes of a picture's record
    int32_t src_at, rows;             // the source's first plane within a record; output rows per wave (strip route: one count for the launch)
    int32_t first[kLanczosPlanarLadderMaxRungs];       // first_block of rung k of this launch (INT_MAX beyond the last): what the scan reads
    PlanarLadderRung rung[kLanczosPlanarLadderMaxRungs];
    PlanarPlane pl[kLanczosPlanarLadderMaxRungs * kLanczosPlanarMaxPlanes];      // rung k's plane p at [k * kLanczosPlanarMaxPlanes + p]; dst / src: sizes only
};
static_assert(sizeof(PlanarLadderArgs) <= 4096 - 256, "kernel arguments: 4 KB in all, 256 bytes of them the runtime's");

struct PlanarLadderBlock {
    PlanarPlane g;
    int T, bx, by;
    bool live;
};

// the rung whose range holds block b: first[] ascends, first[0] == 0
CHV_DEV int planar_ladder_rung_of(const PlanarLadderArgs &a, int b) {
    int r = 0;
#pragma unroll
    for (int k = 1; k < kLanczosPlanarLadderMaxRungs; k++) r = b >= a.first[k] ? k : r;
    return r;
}

// (rung, picture, plane, row chunk, strip) of block b of the grid; dst / src from the descriptor list (scalar loads).  XCD: the XCD-aware
// numbering of planar_lanczos_strip<T> inside the rung's range.
template <bool XCD>
CHV_DEV PlanarLadderBlock planar_ladder_decode(const PlanarLadderArgs &a, int blk) {
    const uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const int r = planar_ladder_rung_of(a, blk);
    const PlanarLadderRung R = cld<PlanarLadderRung>(ka + offsetof(PlanarLadderArgs, rung) + (uint64_t)r * sizeof(PlanarLadderRung));
    PlanarLadderBlock o;
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
    const uint64_t recs = ka + offsetof(PlanarLadderArgs, pl) + (uint64_t)r * kLanczosPlanarMaxPlanes * sizeof(PlanarPlane);
    const int f1 = cld<int32_t>(recs + sizeof(PlanarPlane) + offsetof(PlanarPlane, first));
    const int f2 = cld<int32_t>(recs + 2 * sizeof(PlanarPlane) + offsetof(PlanarPlane, first));
    const int plane = (a.n_planes > 2 && rem >= f2) ? 2 : rem >= f1 ? 1 : 0;
    o.g = cld<PlanarPlane>(recs + (uint64_t)plane * sizeof(PlanarPlane));
    const int in_plane = rem - o.g.first;
    o.by = in_plane / o.g.strips;
    o.bx = in_plane - o.by * o.g.strips;
    const uint64_t pic = (uint64_t)(uintptr_t)a.batch + (uint64_t)picture * a.per_image * sizeof(DPlane);
    o.g.dst = cld<DPlane>(pic + (uint64_t)(R.dst_at + plane) * sizeof(DPlane));
    o.g.src = cld<DPlane>(pic + (uint64_t)(a.src_at + plane) * sizeof(DPlane));
    return o;
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

// one rung of one route, before the launch's order is known
struct PlanarLadderPending {
    PlanarLadderRung R;
    PlanarPlane pl[kLanczosPlanarMaxPlanes];
};

// the records of one launch, largest range first; false when the grid would not fit 30 bits
static bool planar_ladder_order(PlanarLadderArgs *a, const PlanarLadderPending *rungs, int n, int pad, unsigned *grid) {
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

static hipError_t launch_lanczos_planar_ladder(const LanczosPlanarLadderJob &job, hipStream_t stream, int *launches) {
    *launches = 0;
    const int np = job.n_planes;
    if ((np != 2 && np != 3) || job.n_pictures < 1 || job.n_rungs < 1 || job.n_rungs > kLanczosPlanarLadderMaxRungs || !job.batch) return hipErrorInvalidValue;
    // every rung's route and numbers before anything is launched: one refused rung refuses the ladder
    PlanarLadderPending strip[kLanczosPlanarLadderMaxRungs], tile[kLanczosPlanarLadderMaxRungs];
    int strip_nv[kLanczosPlanarLadderMaxRungs];
    int n_strip = 0, n_tile = 0, max_t = 0;
    size_t tile_lds = 0;
    long work = 0;
    for (int r = 0; r < job.n_rungs; r++) {
        const LanczosPlanarLadderRung &j = job.rung[r];
        PlanarLadderPending P{};
        for (int p = 0; p < np; p++) {
            const LanczosPlaneTables &t = j.tab[p];
            const int comps = np == 2 && p == 1 ? 2 : 1;
            PlanarPlane &g = P.pl[p];
            g.fx = t.fx; g.wx = t.wx; g.fy = t.fy; g.wy = t.wy; g.tx = t.tx; g.ty = t.ty;
            g.dst = DPlane{ nullptr, j.w[p], j.h[p], 0, comps };
            g.src = DPlane{ nullptr, job.src_w[p], job.src_h[p], 0, comps };
            if (g.dst.w < 1 || g.dst.h < 1 || g.src.w < 1 || g.src.h < 1 || planar_refuses(g.dst, g.src, t.tx, t.ty)) return hipErrorInvalidValue;
        }
        P.R.dst_at = r * np;
        int T = 0, nvmax = 0;
        if (planar_strip_route(P.pl, np, &T, &nvmax)) {
            P.R.T = T;
            work += planar_strip_work(P.pl, np) * job.n_pictures;
            max_t = std::max(max_t, T);
            strip_nv[n_strip] = nvmax;
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
    // rows per wave from the whole launch's strip work (planar_lanczos_strip<T>'s rule over the sum): one count for every rung
    const int rows = planar_strip_rows(work);
    size_t strip_lds = 0;
    for (int k = 0; k < n_strip; k++) {
        PlanarLadderPending &P = strip[k];
        P.R.per_picture = planar_strip_blocks(P.pl, np, rows);
        const long total = (long)P.R.per_picture * job.n_pictures;
        if (total > 0x3fffffff) return hipErrorInvalidValue;
        P.R.total = (int32_t)total;
        strip_lds = std::max(strip_lds, planar_wtab_bytes(rows, P.R.T) + (size_t)2 * strip_nv[k] * 16);
    }
    PlanarLadderArgs a{};
    a.batch = job.batch; a.n_planes = np; a.per_image = (job.n_rungs + 1) * np; a.src_at = job.n_rungs * np; a.rows = rows;
    PlanarLadderArgs t = a;
    unsigned strip_grid = 0, tile_grid = 0;
    if (n_strip && !planar_ladder_order(&a, strip, n_strip, 8, &strip_grid)) return hipErrorInvalidValue;
    if (n_tile && !planar_ladder_order(&t, tile, n_tile, 1, &tile_grid)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    if (n_strip) {
        if (max_t <= 12) hipLaunchKernelGGL(planar_lanczos_ladder<12>, dim3(strip_grid), dim3(64), strip_lds, stream, a);
        else hipLaunchKernelGGL(planar_lanczos_ladder<22>, dim3(strip_grid), dim3(64), strip_lds, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
    }
    if (n_tile) {
        hipLaunchKernelGGL(planar_lanczos_ladder_tile, dim3(tile_grid), dim3(256), tile_lds, stream, t);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
    }
    return hipSuccess;
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosPlanarLadderRegistrar { LanczosPlanarLadderRegistrar() { register_lanczos_planar_ladder_launcher(launch_lanczos_planar_ladder); } } g_lanczos_planar_ladder_registrar;

}  // namespace chv
