// lanczos_planar_ladder_body.hip.h — what the ladder units of 4:2:0 targets share (kernels_lanczos_planar_ladder.hip.cpp,
// kernels_lanczos_420.hip.cpp, kernels_lanczos_to_420.hip.cpp): how a block finds its target plane, and how a
// ladder's rungs become the arguments of its two launches.  The row code is lanczos_planar_body.hip.h's and its descendants'.
//
// A unit's Args — the type stays its own: its kernels' names carry it — has batch, n_planes, per_image, src_at, rows, first[], rung[]
// (LadderRung420) and pl[] (rung k's target plane p at [k * kLanczosPlanarMaxPlanes + p]; dst / src: sizes only).  Up to 8 rungs x 3 planes
// of records: more than the 1 KB other units allow themselves, inside the 4 KB a launch may carry (the runtime's own hidden arguments take
// 256 bytes of those).  The records are read through the scalar unit at a uniform index, never from a private copy.
#pragma once
#include "lanczos_planar_body.hip.h"
#include "lanczos_planar_ladder.h"
#include "lanczos_ladder_launch.hip.h"

namespace chv {

// What a block works on.  A unit whose target planes read more than one source plane has a record of its own with these members (in this
// order: the kernels' code follows it) and what it adds behind g.
struct PlanarLadderBlock {
    PlanarPlane g;                    // g.dst, g.src: the picture's
    int T, bx, by, plane;             // the rung's tap class; strip and row chunk (tile: tile and tile row); the target plane
    bool live;
};

// (rung, picture, target plane, row chunk, strip) of block blk of the grid; g.dst from the descriptor list (scalar loads).  XCD: the
// XCD-aware numbering of planar_lanczos_strip<T> inside the rung's range.  sources(a, o, pic) loads the source plane or planes that feed
// target plane o.plane — o.g.src and what the unit's Block adds — from the picture's record at pic.
template <bool XCD, class Block, class Args, class Sources>
CHV_DEV Block planar_ladder_block(const Args &a, int blk, Sources sources) {
    const uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const int r = ladder_rung_of(a.first, blk);
    const LadderRung420 R = cld<LadderRung420>(ka + offsetof(Args, rung) + (uint64_t)r * sizeof(LadderRung420));
    Block o;
    o.T = R.T;
    const LadderItem it = ladder_item<XCD>(blk - R.first_block, R.total);
    o.live = it.live;
    if (!o.live) return o;
    const int picture = it.idx / R.per_picture, rem = it.idx - picture * R.per_picture;
    const uint64_t recs = ka + offsetof(Args, pl) + (uint64_t)r * kLanczosPlanarMaxPlanes * sizeof(PlanarPlane);
    const int f1 = cld<int32_t>(recs + sizeof(PlanarPlane) + offsetof(PlanarPlane, first));
    const int f2 = cld<int32_t>(recs + 2 * sizeof(PlanarPlane) + offsetof(PlanarPlane, first));
    o.plane = (a.n_planes > 2 && rem >= f2) ? 2 : rem >= f1 ? 1 : 0;
    o.g = cld<PlanarPlane>(recs + (uint64_t)o.plane * sizeof(PlanarPlane));
    const int in_plane = rem - o.g.first;
    o.by = in_plane / o.g.strips;
    o.bx = in_plane - o.by * o.g.strips;
    const uint64_t pic = (uint64_t)(uintptr_t)a.batch + (uint64_t)picture * a.per_image * sizeof(DPlane);
    o.g.dst = cld<DPlane>(pic + (uint64_t)(R.dst_at + o.plane) * sizeof(DPlane));
    sources(a, o, pic);
    return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// The host half.

// a target plane's record before its route is known: the tables, and dst / src with sizes and component counts
inline PlanarPlane planar_ladder_plane(const LanczosPlaneTables &t, const DPlane &dst, const DPlane &src) {
    PlanarPlane g{};
    g.fx = t.fx; g.wx = t.wx; g.fy = t.fy; g.wy = t.wy; g.tx = t.tx; g.ty = t.ty;
    g.dst = dst; g.src = src;
    return g;
}

// one rung of one route, before the launch's order is known
struct PlanarLadderPending {
    LadderRung420 R;
    PlanarPlane pl[kLanczosPlanarMaxPlanes];
};

// the two launches of a ladder: the strip route's (n_strip rungs; max_t: their largest tap class) and the tile route's
template <class Args>
struct PlanarLadderPlan {
    Args strip, tile;
    int n_strip, n_tile, max_t;
    unsigned strip_grid, tile_grid;
    size_t strip_lds, tile_lds;       // dynamic LDS: the maximum over the launch's rungs
};

// Every rung's route and numbers before anything is launched: false when one rung is refused, which refuses the ladder.  proto: the unit's
// arguments but for rows, first[], rung[] and pl[]; plane(r, p): target plane p of rung r (planar_ladder_plane); route: the unit's strip
// route predicate (planar_strip_route's signature).
template <class Args, class Plane>
inline bool planar_ladder_plan(PlanarLadderPlan<Args> *L, const Args &proto, int n_rungs, int np, int n_pictures, Plane plane,
                               bool (*route)(PlanarPlane *, int, int *, int *)) {
    PlanarLadderPending strip[kLanczosPlanarLadderMaxRungs], tile[kLanczosPlanarLadderMaxRungs];
    int strip_ring[kLanczosPlanarLadderMaxRungs];
    L->n_strip = L->n_tile = L->max_t = 0;
    L->strip_grid = L->tile_grid = 0;
    L->strip_lds = L->tile_lds = 0;
    long work = 0;
    for (int r = 0; r < n_rungs; r++) {
        PlanarLadderPending P{};
        for (int p = 0; p < np; p++) {
            PlanarPlane &g = P.pl[p];
            g = plane(r, p);
            if (g.dst.w < 1 || g.dst.h < 1 || g.src.w < 1 || g.src.h < 1 || lanczos_refuses(g.dst.w, g.dst.h, g.src.w, g.src.h, g.tx, g.ty)) return false;
        }
        P.R.dst_at = r * np;
        int T = 0, ring = 0;
        if (route(P.pl, np, &T, &ring)) {
            P.R.T = T;
            work += planar_strip_work(P.pl, np) * n_pictures;
            L->max_t = std::max(L->max_t, T);
            strip_ring[L->n_strip] = ring;
            strip[L->n_strip++] = P;
        } else {
            int rows_max = 0;
            P.R.per_picture = planar_tile_blocks(P.pl, np, &rows_max);
            const long total = (long)P.R.per_picture * n_pictures;
            const size_t lds = (size_t)rows_max * PT_W * sizeof(float);
            if (total > 0x3fffffff || lds > 64 * 1024) return false;
            P.R.total = (int32_t)total;
            L->tile_lds = std::max(L->tile_lds, lds);
            tile[L->n_tile++] = P;
        }
    }
    // rows per wave from the whole launch's strip work (planar_lanczos_strip<T>'s rule over the sum): one count for every rung.  The strip
    // body finds its staging ring behind a weight table of ITS OWN tap class.
    const int rows = lanczos_strip_rows(work, PS_MAX_ROWS);
    for (int k = 0; k < L->n_strip; k++) {
        PlanarLadderPending &P = strip[k];
        P.R.per_picture = planar_strip_blocks(P.pl, np, rows);
        const long total = (long)P.R.per_picture * n_pictures;
        if (total > 0x3fffffff) return false;
        P.R.total = (int32_t)total;
        L->strip_lds = std::max(L->strip_lds, lanczos_wtab_bytes(rows, P.R.T) + (size_t)2 * strip_ring[k] * 16);
    }
    L->strip = proto;
    L->strip.rows = rows;
    L->tile = L->strip;
    const auto total = [](const PlanarLadderPending &P) { return P.R.total; };
    const auto copy = [](Args *a, int k, const PlanarLadderPending &P) {
        a->rung[k] = P.R;
        for (int p = 0; p < kLanczosPlanarMaxPlanes; p++) a->pl[k * kLanczosPlanarMaxPlanes + p] = P.pl[p];
    };
    return (!L->n_strip || ladder_order(&L->strip, strip, L->n_strip, 8, &L->strip_grid, total, copy)) &&
           (!L->n_tile || ladder_order(&L->tile, tile, L->n_tile, 1, &L->tile_grid, total, copy));
}

}  // namespace chv
