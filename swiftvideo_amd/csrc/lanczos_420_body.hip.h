// lanczos_420_body.hip.h — the row code of the planar Lanczos-3 resampler BETWEEN the two 4:2:0 packings, for
// kernels_lanczos_420.hip.cpp (chv_scale_lanczos_420, chv_scale_lanczos_420_ladder).  The arithmetic is that of lanczos_planar_body.hip.h,
// logical plane by logical plane, so the bytes are; luma IS planar_strip<T, 1>.  What is here is the chroma of the two cross pairs, which
// differ from the same-format bodies in how a lane finds its source bytes and nowhere else:
//
//   x420_strip<T, true>    y420p -> NV12.  The target is the CbCr plane: a strip is 64 output bytes = 32 texels, even lanes filter Cb from source
//                          plane 1, odd lanes Cr from source plane 2.  Every source step stages one row of EACH plane into the ring — loader
//                          lanes < nv load Cb, the next nv load Cr — and a lane's tap offset picks its half.  Tap stride 1.
//   x420_strip<T, false>   NV12 -> y420p.  The target is one of the two 1-component chroma planes (`comp`: 0 Cb, 1 Cr): a strip is 64 texels.
//                          It stages the CbCr row and reads it with a tap stride of two from byte `comp` — the 2-component tap extraction
//                          under 1-component output indexing.  Its staged row is twice as long as the same-format one; x420_strip_route counts that.
//   x420_tile              any tap counts, all three kinds of plane (luma included): planar_tile with the source addressing as parameters.
//
// Both strips are strip_core (lanczos_strip_core.hip.h) under another column description.  THE routing rule of these entries is
// x420_strip_route (lanczos_route.h).
#pragma once
#include "lanczos_planar_body.hip.h"

#pragma clang fp contract(off)

namespace chv {

// One strip of one chroma target plane.  g.src: the CbCr plane (NV12 source) or the Cb plane (y420p source), src2: the Cr plane of a y420p
// source (same width and height as Cb; its own start and pitch).  comp_in: the component a 1-component target takes.
template <int T, bool TO_NV12>
CHV_DEV void x420_strip(const PlanarPlane &g, const DPlane &src2, int comp_in, int strip, int chunk, int rows_per_wave, uint8_t *lsm) {
    // even lanes read the first half of the ring slot (g.src's row), odd lanes the second (src2's), nv vectors on
    if constexpr (TO_NV12) strip_core<T, StripCols<1, 2, true>>(g, src2, 0, g.nv * 16, strip, chunk, rows_per_wave, lsm, OpenByteQuads{});
    else strip_core<T, StripCols<2, 1>>(g, src2, comp_in, 0, strip, chunk, rows_per_wave, lsm, OpenByteQuads{});
}

// ---------------------------------------------------------------------------------------------------------------------
// x420_tile — planar_tile for a logical plane whose source is packed differently: output byte b of a row is texel b / OC (OC = g.dst.comps),
// component b % OC; its source row starts at `sa` (component 0 of the target, or the only one) or `sb` (component 1 of an NV12 target
// fed from a y420p source) and its taps are `stride` bytes apart.
CHV_DEV void x420_tile(const PlanarPlane &g, const uint8_t *sa, int pitch_a, const uint8_t *sb, int pitch_b, int stride, int bx, int by, uint8_t *lsm) {
    float *hrow = (float *)lsm;                                    // [max_rows][PT_W]
    const DPlane dst = g.dst, src = g.src;
    const int32_t *__restrict__ fx = g.fx; const float *__restrict__ wx = g.wx;
    const int32_t *__restrict__ fy = g.fy; const float *__restrict__ wy = g.wy;
    const int tx = g.tx, ty = g.ty, OC = dst.comps;
    const int wb = dst.w * OC;
    const int ox0 = bx * PT_W, oy0 = by * PT_H;
    if (ox0 >= wb || oy0 >= dst.h) return;
    const int oy_last = min(oy0 + PT_H, dst.h) - 1;
    const int row0 = gld<int32_t>(fy + oy0);
    const int nrows = min(gld<int32_t>(fy + oy_last) + ty - row0, g.max_rows);
    const int tid = threadIdx.x;
    for (int e = tid; e < nrows * PT_W; e += 256) {
        const int r = e / PT_W, i = e % PT_W;
        const int xe = min(ox0 + i, wb - 1);
        const int xt = OC == 2 ? xe >> 1 : xe, comp = xe & (OC - 1);
        const int f = gld<int32_t>(fx + xt);
        const float *w = wx + (size_t)xt * tx;
        const size_t sy = (size_t)min(max(row0 + r, 0), src.h - 1);
        const uint8_t *rowp = comp ? sb + sy * pitch_b : sa + sy * pitch_a;
        float acc = 0.f;
        for (int k = 0; k < tx; k++)
            acc = __builtin_fmaf(gld<float>(w + k), (float)gld<uint8_t>(rowp + (size_t)min(max(f + k, 0), src.w - 1) * stride), acc);
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

// (THE routing rule of these entries, x420_strip_route, is lanczos_route.h's)

}  // namespace chv
