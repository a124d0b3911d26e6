// lanczos_hbd_body.hip.h — the row code of the planar Lanczos-3 resampler for 10-bit sources, for
// kernels_lanczos_hbd.hip.cpp (chv_scale_lanczos_hbd_to_420, chv_scale_lanczos_hbd_to_420_ladder).  The arithmetic is that of
// lanczos_planar_body.hip.h, logical image by logical image, on the 10-bit codes; one step is new: the value that leaves the vertical chain
// is multiplied by 0.25f (exact) before the one rounding to a byte.  The strips are strip_core (lanczos_strip_core.hip.h) under column
// descriptions with a 16-bit sample; the tile is x420_tile with a 16-bit load.
//
//   hbd_strip<T, 2, 1, false, W>   a plane of 16-bit samples into a 1-component plane: every luma, the chroma of y420p10 -> y420p.
//   hbd_strip<T, 4, 1, false, W>   one word of P010's CbCr texels (byte offset 0 or 2) into one chroma plane of y420p.
//   hbd_strip<T, 4, 2, false, W>   P010's CbCr plane into NV12's: even lanes read word 0, odd lanes word 1.
//   hbd_strip<T, 2, 2, true, W>    the Cb and Cr planes of y420p10 into NV12's CbCr plane: one staged row of each in a ring slot.
#pragma once
#include "lanczos_420_body.hip.h"

#pragma clang fp contract(off)

namespace chv {

// ByteQuadSink behind the final scaling: 10-bit code scale -> 8-bit code scale.  The product is exact (a power of two, no underflow: the
// chain's values are sums of codes times weights), so v_cvt_pk_u8_f32 still rounds once.
struct HbdQuadSink {
    ByteQuadSink bytes;
    CHV_DEV void operator()(int jcur, float o) const { bytes(jcur, o * 0.25f); }
};
struct OpenHbdQuads {
    CHV_DEV HbdQuadSink operator()(const DPlane &dst, int wb, int xb, int j0) const { return HbdQuadSink{ ByteQuadSink(dst, wb, xb, j0) }; }
};

// One strip of one target plane of OC components, fed from 16-bit samples SS bytes apart.  g.src: the LOGICAL image's size (samples), the
// start and pitch of the plane that holds it; src2: with TWO the plane of the odd lanes' image.  off0, off1: even.
template <int T, int SS, int OC, bool TWO, int WIDE>
CHV_DEV void hbd_strip(const PlanarPlane &g, const DPlane &src2, int off0, int off1, int strip, int chunk, int rows_per_wave, uint8_t *lsm) {
    static_assert(WIDE == kSampleHigh10 || WIDE == kSampleLow10, "a 16-bit sample");
    strip_core<T, StripCols<SS, OC, TWO, WIDE>>(g, src2, off0, off1, strip, chunk, rows_per_wave, lsm, OpenHbdQuads{});
}

// ---------------------------------------------------------------------------------------------------------------------
// hbd_tile — x420_tile for 16-bit samples: the source row of component 0 of the target (or the only one) starts at `sa`, of component 1 at
// `sb`; samples are `stride` bytes apart (all even) and their code is (word >> shift) & 1023 — shift 6 for P010, 0 for y420p10.
CHV_DEV void hbd_tile(const PlanarPlane &g, const uint8_t *sa, int pitch_a, const uint8_t *sb, int pitch_b, int stride, int shift, int bx, int by, uint8_t *lsm) {
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
        for (int k = 0; k < tx; k++) {
            const uint32_t word = gld<uint16_t>((const uint16_t *)(rowp + (size_t)min(max(f + k, 0), src.w - 1) * stride));
            acc = __builtin_fmaf(gld<float>(w + k), (float)((word >> shift) & 1023u), acc);
        }
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
            gst<uint8_t>(dst.ptr + (size_t)oy * dst.pitch + xb, (uint8_t)to_code_raw(acc * 0.25f));
        }
    }
}

}  // namespace chv
