// lanczos_from_yuv_body.hip.h — the row code of the Lanczos-3 resampler FROM a 4:2:0 picture INTO a BGRA / RGBA plane (DESIGN.md section
// 4.4.6), for kernels_lanczos_from_yuv.hip.cpp (chv_scale_lanczos_from_yuv, chv_scale_lanczos_from_yuv_batch).  Every logical plane (Y, Cb,
// Cr) is resampled to the TARGET's size by the arithmetic of lanczos_planar_body.hip.h and rounded to a code; the three codes of a pixel go
// through the integer matrix of section 4.2.  Nothing crosses from one plane into another before its code is rounded, so the order in which a
// block resamples its planes is free:
//
//   fy_strip<T, SC>   one strip of one logical plane: 64 output columns x `rows` output rows — strip_core (lanczos_strip_core.hip.h), as
//                     planar_strip<T, 1> / x420_strip<T, false> are.  SC is the tap stride: 1 for a plane of its own, 2 for component `comp`
//                     of an NV12 picture's CbCr plane.  What differs is where a finished output value goes: to the caller's
//                     `sink(row, value)`, not to memory.  A wave runs it three times over the same block: Cb
//                     and Cr leave their codes in LDS (fy_code_sink), luma takes its lane's two codes back, applies the matrix and stores
//                     one dword per lane — 256 contiguous bytes per wave and row (fy_pixel_sink).  A lane only ever reads the codes it wrote.
//   fy_tile_plane     any tap counts: planar_tile's two passes for one logical plane of a 32 x 4 pixel tile, the result returned as a code.
//
// The host half — the routing rule and the launch numbers — is at the end.
#pragma once
#include "lanczos_420_body.hip.h"

#pragma clang fp contract(off)

namespace chv {

// One strip of one logical plane.  g.dst: the TARGET's width and height with one component (its pointer is not used), g.src: the plane that
// holds the logical plane, of SC components; comp: the component.  sink(row of the chunk, value): the plane's value of column ox0 + lane,
// before rounding.
template <int T, int SC, typename Sink>
CHV_DEV void fy_strip(const PlanarPlane &g, int comp, int strip, int chunk, int rows_per_wave, uint8_t *lsm, Sink &&sink) {
    if (!strip_core<T, StripCols<SC, 1>>(g, g.src, comp, 0, strip, chunk, rows_per_wave, lsm, [&](const DPlane &, int, int, int) -> Sink & { return sink; })) return;
    // the next plane of this block reuses the weights' and the ring's LDS: nothing of this pass may move behind its first write
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
}

// section 4.2 on three codes, plain form; the memory-order word of a BGRA target, or of an RGBA one (red and blue exchanged)
CHV_DEV uint32_t fy_pixel(const Csc &k, bool rgba, int y, int u, int v) {
    const int32_t c = k.cy * (y - k.yoff) + 32768;
    const int32_t d = u - 128, e = v - 128;
    const int32_t r = c + k.crv * e, gg = c - k.cgu * d - k.cgv * e, b = c + k.cbu * d;
    return rgba ? pack_bgra_fixed(r, gg, b) : pack_bgra_fixed(b, gg, r);
}

// ---------------------------------------------------------------------------------------------------------------------
// fy_tile_plane — planar_tile's two passes for one logical plane of the tile (bx, by) of 32 x 4 TARGET pixels: `sa` is the plane's first
// byte (component included), its taps are `stride` bytes apart.  Returns the code of pixel (ox0 + tid % 32, oy0 + tid / 32) to threads
// tid < 128 inside the picture, 0 to the others.  Every thread of the block must call it: it holds two block barriers, the first one so
// that the previous plane's vertical pass has left the LDS array.
CHV_DEV uint32_t fy_tile_plane(const PlanarPlane &g, const uint8_t *sa, int pitch, int stride, int bx, int by, uint8_t *lsm) {
    float *hrow = (float *)lsm;                                    // [max_rows][PT_W]
    const DPlane dst = g.dst, src = g.src;
    const int32_t *__restrict__ fx = g.fx; const float *__restrict__ wx = g.wx;
    const int32_t *__restrict__ fy = g.fy; const float *__restrict__ wy = g.wy;
    const int tx = g.tx, ty = g.ty;
    const int ox0 = bx * PT_W, oy0 = by * PT_H;
    const int oy_last = min(oy0 + PT_H, dst.h) - 1;
    const int row0 = gld<int32_t>(fy + oy0);
    const int nrows = min(gld<int32_t>(fy + oy_last) + ty - row0, g.max_rows);
    const int tid = threadIdx.x;
    __syncthreads();
    for (int e = tid; e < nrows * PT_W; e += 256) {
        const int r = e / PT_W, i = e % PT_W;
        const int xt = min(ox0 + i, dst.w - 1);
        const int f = gld<int32_t>(fx + xt);
        const float *w = wx + (size_t)xt * tx;
        const uint8_t *rowp = sa + (size_t)min(max(row0 + r, 0), src.h - 1) * pitch;
        float acc = 0.f;
        for (int k = 0; k < tx; k++)
            acc = __builtin_fmaf(gld<float>(w + k), (float)gld<uint8_t>(rowp + (size_t)min(max(f + k, 0), src.w - 1) * stride), acc);
        hrow[e] = acc;
    }
    __syncthreads();
    uint32_t code = 0;
    if (tid < PT_W * PT_H) {
        const int i = tid % PT_W, j = tid / PT_W;
        const int oy = oy0 + j;
        if (ox0 + i < dst.w && oy < dst.h) {
            const int rbase = gld<int32_t>(fy + oy) - row0;
            const float *w = wy + (size_t)oy * ty;
            float acc = 0.f;
            for (int k = 0; k < ty; k++) acc = __builtin_fmaf(gld<float>(w + k), hrow[(rbase + k) * PT_W + i], acc);
            code = to_code_raw(acc);
        }
    }
    return code;
}

// ---------------------------------------------------------------------------------------------------------------------
// The host half.  `pl`: the logical planes luma [0] and chroma [1] (Cb and Cr have one size, so one record) with dst (the target's size, one
// component), src (the plane's size; comps 2 for the CbCr plane of NV12), tx and ty filled in.

constexpr int FY_MAX_ROWS = 32;      // output rows per wave at most: two codes per pixel of the block wait in LDS besides the weights

// THE routing rule of chv_scale_lanczos_from_yuv (it reads no switch): x420_strip_route's on the logical planes — the strip route when no
// plane has more than 22 taps on an axis and no ring slot is longer than 64 vectors.  *TL, *TC: the tap classes of luma and of chroma, each
// over its own tap counts; every plane's nv is set.  Chroma never has more than 12 taps on the strip route: its scale is at most half the
// luma's (cw = iw / 2 rounded down, or both are 1), 22 luma taps mean a scale of at most 11 / 3, and 2 ceil(3 x 11 / 6) = 12.  The kernels
// hold chroma bodies up to 12 taps only, so the rule says it all the same.
inline bool fy_strip_route(PlanarPlane *pl, int *TL, int *TC, int *ring_max) {
    int T = 0;
    if (!x420_strip_route(pl, 2, &T, ring_max)) return false;
    *TL = lanczos_tap_class(std::max(pl[0].tx, pl[0].ty));
    *TC = lanczos_tap_class(std::max(pl[1].tx, pl[1].ty));
    return *TC <= 12;
}

// rows per wave: lanczos_strip_rows on the (strip, output row) pairs of the launch
inline int fy_strip_rows(long work) { return lanczos_strip_rows(work, FY_MAX_ROWS); }

// LDS of one wave on the strip route: the vertical weights of the widest body, the longest ring, the codes of Cb and Cr
inline size_t fy_codes_at(int rows, int TL, int TC, int ring_max) { return lanczos_wtab_bytes(rows, std::max(TL, TC)) + (size_t)2 * ring_max * 16; }
inline size_t fy_strip_lds(int rows, int TL, int TC, int ring_max) { return fy_codes_at(rows, TL, TC, ring_max) + (size_t)2 * 64 * rows; }

}  // namespace chv
