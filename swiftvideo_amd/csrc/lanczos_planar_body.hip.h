// lanczos_planar_body.hip.h — the row code of the planar Lanczos-3 resampler, shared by the units that launch it:
// kernels_lanczos_planar.hip.cpp (chv_scale_lanczos on NV12 / y420p pictures: one geometry per launch) and
// kernels_lanczos_planar_ladder.hip.cpp (chv_scale_lanczos_ladder: up to eight geometries per launch).  What differs between the two is how a
// block finds its work; the bytes come from here.
//
// Both bodies see a plane as rows of BYTE columns: output byte b of a row belongs to texel b / C, component b % C, and its taps are the
// source bytes (first[b / C] + k) * C + b % C — a stride of C bytes.  A 2-component plane is therefore the 1-component body with a tap
// stride of two, and one lane owns one output byte whatever the plane is.
//
//   planar_strip<T, C>   every tap count of the launch's geometry <= T <= 22: strip_core (lanczos_strip_core.hip.h) with a tap stride of C
//                        bytes into a target of C bytes per texel, one source plane, a dword store per quad.
//   planar_tile          everything else: 32 x 4 output bytes per 256-thread block, horizontal pass from global memory into LDS, vertical
//                        pass out of it.  Simple on purpose.
//
// The host half — which route a geometry takes, its launch numbers — is here too, so that no launcher restates it.
#pragma once
#include "lanczos_strip_core.hip.h"
#include "lanczos_planar.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace chv {

// One strip of one plane with C components: 64 output BYTE columns, rows [chunk * rows, ...)
template <int T, int C>
CHV_DEV void planar_strip(const PlanarPlane &g, int strip, int chunk, int rows_per_wave, uint8_t *lsm) {
    strip_core<T, StripCols<C, C>>(g, g.src, 0, 1, strip, chunk, rows_per_wave, lsm, OpenByteQuads{});      // component b % C from component b % C
}

// ---------------------------------------------------------------------------------------------------------------------
// planar_tile — any tap counts.  A block makes 32 output byte columns x 4 output rows: the horizontal pass reads its taps from global
// memory (CLAMP_TO_EDGE on the texel index) and leaves one float per (source row, column) in LDS, the vertical pass runs out of it.
constexpr int PT_W = 32, PT_H = 4;

CHV_DEV void planar_tile(const PlanarPlane &g, int bx, int by, uint8_t *lsm) {
    float *hrow = (float *)lsm;                                    // [max_rows][PT_W]
    const DPlane dst = g.dst, src = g.src;
    const int32_t *__restrict__ fx = g.fx; const float *__restrict__ wx = g.wx;
    const int32_t *__restrict__ fy = g.fy; const float *__restrict__ wy = g.wy;
    const int tx = g.tx, ty = g.ty, C = dst.comps;
    const int wb = dst.w * C;
    const int ox0 = bx * PT_W, oy0 = by * PT_H;
    if (ox0 >= wb || oy0 >= dst.h) return;
    const int oy_last = min(oy0 + PT_H, dst.h) - 1;
    const int row0 = gld<int32_t>(fy + oy0);
    const int nrows = min(gld<int32_t>(fy + oy_last) + ty - row0, g.max_rows);
    const int tid = threadIdx.x;
    for (int e = tid; e < nrows * PT_W; e += 256) {
        const int r = e / PT_W, i = e % PT_W;
        const int xe = min(ox0 + i, wb - 1);
        const int xt = C == 2 ? xe >> 1 : xe, comp = xe & (C - 1);
        const int f = gld<int32_t>(fx + xt);
        const float *w = wx + (size_t)xt * tx;
        const uint8_t *rowp = src.ptr + (size_t)min(max(row0 + r, 0), src.h - 1) * src.pitch + comp;
        float acc = 0.f;
        for (int k = 0; k < tx; k++)
            acc = __builtin_fmaf(gld<float>(w + k), (float)gld<uint8_t>(rowp + (size_t)min(max(f + k, 0), src.w - 1) * C), acc);
        hrow[e] = acc;
    }
    __syncthreads();
    if (tid < PT_W * PT_H) {
        const int i = tid % PT_W, j = tid / PT_W;
        const int xb = ox0 + i, oy = oy0 + j;
        if (xb < wb && oy < dst.h) {
            const int rbase = gld<int32_t>(fy + oy) - row0;
            const float *w = wy + (size_t)oy * ty;
            float acc = 0.f;
            for (int k = 0; k < ty; k++) acc = __builtin_fmaf(gld<float>(w + k), hrow[(rbase + k) * PT_W + i], acc);
            gst<uint8_t>(dst.ptr + (size_t)oy * dst.pitch + xb, (uint8_t)to_code_raw(acc));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The host half: one geometry's route and launch numbers.  `pl`: the np planes of one picture with dst, src (sizes and component counts),
// tx and ty filled in.

// (the refusal, THE routing rule planar_strip_route and the rows-per-wave rule are lanczos_route.h's: no HIP, so a CPU test walks them)

// strip route: every plane's strips; the (strip, output row) pairs of one picture
inline long planar_strip_work(PlanarPlane *pl, int np) {
    long work = 0;
    for (int p = 0; p < np; p++) {
        pl[p].strips = (pl[p].dst.w * pl[p].dst.comps + 63) / 64;
        work += (long)pl[p].strips * pl[p].dst.h;
    }
    return work;
}

// strip route: every plane's chunks and first; the blocks of one picture
inline int planar_strip_blocks(PlanarPlane *pl, int np, int rows) {
    int first = 0;
    for (int p = 0; p < np; p++) {
        pl[p].chunks = (pl[p].dst.h + rows - 1) / rows;
        pl[p].first = first;
        first += pl[p].strips * pl[p].chunks;
    }
    return first;
}

// tile route: every plane's strips, chunks, max_rows and first; the blocks of one picture, *rows_max the longest LDS array
inline int planar_tile_blocks(PlanarPlane *pl, int np, int *rows_max) {
    int first = 0;
    *rows_max = 0;
    for (int p = 0; p < np; p++) {
        PlanarPlane &g = pl[p];
        const double sy = (double)g.src.h / (double)g.dst.h;
        g.strips = (g.dst.w * g.dst.comps + PT_W - 1) / PT_W;
        g.chunks = (g.dst.h + PT_H - 1) / PT_H;
        g.max_rows = (int)((PT_H - 1) * sy + 2) + g.ty;
        *rows_max = std::max(*rows_max, g.max_rows);
        g.first = first;
        first += g.strips * g.chunks;
    }
    return first;
}

}  // namespace chv
