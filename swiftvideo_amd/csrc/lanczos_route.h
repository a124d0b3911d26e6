// lanczos_route.h — the integer rules every Lanczos-3 unit's host half asks, for the host and for g++ alone (no HIP in
// here: tests/cpp/test_lanczos_route.cpp pins their answers to tables on the CPU).
#pragma once
#include "device_types.h"

#include <stddef.h>

#include <algorithm>

namespace chv {

// a strip body's tap class: the smallest of 6 / 8 / 12 / 16 / 22 over a geometry's largest tap count (the padding costs (T - taps) / taps of
// the arithmetic; a count above 22 takes the tile route, whatever this says)
inline int lanczos_tap_class(int tmax) { return tmax <= 6 ? 6 : tmax <= 8 ? 8 : tmax <= 12 ? 12 : tmax <= 16 ? 16 : 22; }

// rows per wave of a strip launch from its (strip, output row) pairs: enough waves for three rounds of four per SIMD when the launch is large; a
// small launch gets short chunks instead — every chunk re-filters ty - 2 warm-up rows, but a wave's serial chain is what a lone resize waits
// for.  `most`: what the body's LDS holds.
inline int lanczos_strip_rows(long work, int most) {
    const long want = 4L * 1024 * 3;
    const long r = (work + want - 1) / want;
    return (int)std::min<long>(std::max<long>(r, 8), most);
}

// chv_scale_lanczos's refusal (launch_lanczos: the 8 x 4 tile's staged source beyond 160 KB), evaluated on one image's own sizes.  Every
// Lanczos entry refuses what the 4-component one would: no strip-route geometry comes near it.
inline bool lanczos_refuses(int dw, int dh, int sw, int sh, int tx, int ty) {
    const double sy = (double)sh / (double)dh, sx = (double)sw / (double)dw;
    const int max_rows = (int)(3 * sy + 2) + ty;
    const int max_cols = ((int)(7 * sx + 2) + tx + 3) & ~3;
    return (size_t)max_rows * 8 * 16 + (size_t)max_rows * max_cols * 4 > 160 * 1024;
}

// what a block of the planar units needs to know about the plane it works on (kernel arguments: read through the constant address space with
// the plane's index, never by indexing a private copy of the argument)
struct PlanarPlane {
    const int32_t *fx; const float *wx;
    const int32_t *fy; const float *wy;
    DPlane dst, src;                  // picture 0's (a batch reads its own from the descriptor list)
    int32_t tx, ty;
    int32_t strips, chunks;           // blocks along x and y
    int32_t nv;                       // strip kernel: 16-byte vectors of one staged source row
    int32_t max_rows;                 // tile kernel: rows of the LDS array
    int32_t first;                    // blocks of this picture's planes in front of this one
    int32_t pad;
};

// THE routing rule of the planar units (they read no switch).  `pl`: the np target planes of one geometry with dst, src (sizes and component
// counts: src.comps is what the source plane that feeds this target plane has), tx and ty filled in.  Strip route (true): no plane has more
// than 22 taps on an axis and no ring slot is longer than 64 vectors.  A target plane of OC components fed from a plane of SC stages the span
// of its 64 / OC texel columns in SC bytes per texel, and a CbCr target fed from two 1-component planes stages one such row of each.  *T:
// the body's tap class over the geometry's largest tap count; every plane's nv (vectors of ONE staged row) is set, *ring_max is the longest
// ring slot.  Tile route otherwise.
inline bool x420_strip_route(PlanarPlane *pl, int np, int *T, int *ring_max) {
    int tmax = 0;
    for (int p = 0; p < np; p++) tmax = std::max(tmax, std::max(pl[p].tx, pl[p].ty));
    *T = lanczos_tap_class(tmax);
    *ring_max = 0;
    if (tmax > 22) return false;
    for (int p = 0; p < np; p++) {
        PlanarPlane &g = pl[p];
        const int OC = g.dst.comps, SC = g.src.comps;
        const double sx = (double)g.src.w / (double)g.dst.w;
        // first[x + n] - first[x] <= floor(n scale) + 1 texels over the strip's 64 / OC texel columns; 15 bytes of alignment in front,
        // the dword reads of the last column (its T taps, rounded out to dwords) behind
        const int span = ((int)((64 / OC - 1) * sx) + 1) * SC + (SC - 1);
        const int bytes = 15 + span + 4 * (((*T * SC - SC + 7) / 4) + 1);
        g.nv = (bytes + 15) / 16 + 1;
        *ring_max = std::max(*ring_max, OC == 2 && SC == 1 ? 2 * g.nv : g.nv);
    }
    return *ring_max <= 64;
}
// (same-format planes, src.comps == dst.comps: the ring slot is the staged row)
inline bool planar_strip_route(PlanarPlane *pl, int np, int *T, int *nvmax) { return x420_strip_route(pl, np, T, nvmax); }

}  // namespace chv
