// yuv_rows.hip.h — what a row of a layer computes on a 4:2:0 canvas (NV12, y420p), stated once: tick_yuv_stream (kernels_stream_yuv.hip.cpp)
// runs its rows through these functions, tick_yuv_wave (kernels_wave_yuv.hip.cpp) takes the helpers and shuffles from here.  Bytes: oracle/
// ref_kernels.c::px_yuv_to_yuv / px_rgb_to_yuv / px_rgb_to_yuv_int; the per-pixel statement of record is yuv_pixel.hip.h.  Where the taps lie
// (rectangles, rings, row tables) is the kernels' business: the functions take converted taps, packed texel words and weights.  A kernel that
// needs another FORM of a step (half weights, a matrix through mad24_uniform, a byte position in a register) passes a parameter or keeps that line.
#pragma once
#include "wave_common.hip.h"

#include <type_traits>
#include <utility>

namespace chv {

// ---- code helpers -----------------------------------------------------------------------------------------------------------------
// UNORM8 loads: c / 255.0f, correctly rounded — the two-term product of pixel_math.hip.h (cvt + mul + fma per byte; a single multiply is wrong
// for 126 of 256 codes).  A 256-entry LDS table in their place was measured in rounds 2 and 6 and is gone from the source
// (profiles/r06_unorm_table_experiment.patch, r06_notes.md section 3): it removes 8 % of the launch's vector instructions and is 6 % SLOWER on
// conflict-free content (gradients: 4.9 M bank-conflict cycles), 6-7 % on low-pass noise (34 M), 6-10 % on random bytes (121 M) — an LDS read
// occupies the CU's one LDS pipe for as long as one of its four SIMDs would have spent on the arithmetic.
CHV_DEV float T8(uint32_t byte) { return unorm8(byte); }
// the same for byte K of a packed word
template <int K>
CHV_DEV float T8k(uint32_t w) {
    return unorm8f(K == 0 ? (float)(w & 255u) : K == 1 ? (float)((w >> 8) & 255u) : K == 2 ? (float)((w >> 16) & 255u) : (float)(w >> 24));
}
// code-scale variants (the integer-matrix RGB kind): byte K of a word as a float; to_code_raw of a code-scale value into byte K
// (v_cvt_pk_u8_f32: RTE, clamp to [0, 255], NaN -> 0)
template <int K>
CHV_DEV float ubk(uint32_t w) { return K == 0 ? ub0(w) : K == 1 ? ub1(w) : K == 2 ? ub2(w) : ub3(w); }
template <int K>
CHV_DEV uint32_t put_code_raw(uint32_t w, float v) {
    if (K == 0) asm("v_cvt_pk_u8_f32 %0, %1, 0, %0" : "+v"(w) : "v"(v));
    if (K == 1) asm("v_cvt_pk_u8_f32 %0, %1, 1, %0" : "+v"(w) : "v"(v));
    if (K == 2) asm("v_cvt_pk_u8_f32 %0, %1, 2, %0" : "+v"(w) : "v"(v));
    if (K == 3) asm("v_cvt_pk_u8_f32 %0, %1, 3, %0" : "+v"(w) : "v"(v));
    return w;
}
// convert_uchar_sat_rte(f * 255) into byte K of w (= to_code)
template <int K>
CHV_DEV uint32_t put_code(uint32_t w, float f) { return put_code_raw<K>(w, f * 255.0f); }
// row(integral_constant<int, j>) for j = 0 .. N - 1, in order (the row index is a compile-time constant in the body: byte
// positions of the packed canvas codes are immediates)
template <typename F, int... J>
CHV_DEV void for_each_row_impl(F &f, std::integer_sequence<int, J...>) { (f(std::integral_constant<int, J>{}), ...); }
template <int N, typename F>
CHV_DEV void for_rows(F &f) { for_each_row_impl(f, std::make_integer_sequence<int, N>{}); }

// the even lane's value in both lanes of a column pair (quad_perm [0, 0, 2, 2])
CHV_DEV int quad_even(int v) { return __builtin_amdgcn_update_dpp(v, v, 0xA0, 0xf, 0xf, false); }
CHV_DEV float quad_even(float v) { return __int_as_float(quad_even(__float_as_int(v))); }

// ---- store shuffles ---------------------------------------------------------------------------------------------------------------
// A 4 x 4 byte transpose inside every quad of lanes: "4 rows of one column" (byte r of lane 4 c + i) become "4 columns of one row" (lane
// 4 c + r holds row r, columns 4 c .. 4 c + 3) — a dword store per lane in place of four byte stores
struct QuadSel { uint32_t sel1, sel2; };        // (the v_perm selectors depend on the lane alone: computed once, where the kernel wants them)
CHV_DEV QuadSel quad_sel(int lane) { return QuadSel{ (lane & 1) ? 0x03070105u : 0x06020400u, (lane & 2) ? 0x03020706u : 0x05040100u }; }
CHV_DEV uint32_t quad_transpose(uint32_t v, const QuadSel &s) {
    const uint32_t p1 = (uint32_t)__builtin_amdgcn_update_dpp(dpp_old(), (int)v, 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, false);
    const uint32_t a = __builtin_amdgcn_perm(p1, v, s.sel1);
    const uint32_t p2 = (uint32_t)__builtin_amdgcn_update_dpp(dpp_old(), (int)a, 0x4E /* quad_perm [2,3,0,1] */, 0xf, 0xf, false);
    return __builtin_amdgcn_perm(p2, a, s.sel2);
}
// Chroma codes of 16 canvas rows.  Lane 2k: rows 0, 2, 4, 6 of chroma column k; lane 2k + 1: rows 1, 3, 5, 7  ->  lane 2k: rows 0-3, lane
// 2k + 1: rows 4-7 (v_perm); one ds_bpermute packs the columns (lane 8c + i <- column 4c + i, rows 0-3; lane 8c + 4 + i <- the same column,
// rows 4-7); then the transpose: lane 8c + i holds row i (+ 4 for lanes 8c + 4 ..), columns 4c .. 4c + 3
CHV_DEV uint32_t chroma_regroup(uint32_t v, int lane) {
    const uint32_t selp = (lane & 1) ? 0x03070206u : 0x05010400u;
    const int src = ((lane & ~7) + 2 * (lane & 3) + ((lane >> 2) & 1)) * 4;
    const QuadSel qs = quad_sel(lane);
    const uint32_t p = (uint32_t)__builtin_amdgcn_update_dpp(dpp_old(), (int)v, 0xB1, 0xf, 0xf, false);
    const uint32_t a = __builtin_amdgcn_perm(p, v, selp);
    return quad_transpose((uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)a), qs);
}

// ---- tap weights ------------------------------------------------------------------------------------------------------------------
struct TapWeights { float w00, w10, w01, w11; };           // top row: tap column 0, 1; bottom row: tap column 0, 1
// a, b: weight of tap column 1 / of the bottom row; ia = 1 - a, ib = 1 - b
CHV_DEV TapWeights tap_weights(float a, float ia, float b, float ib) { return TapWeights{ ia * ib, a * ib, ia * b, a * b }; }
// the short form (both column weights one half: a picture drawn at its own size): two products
CHV_DEV TapWeights tap_weights_half(float b, float ib) { const float wt = 0.5f * ib, wb = 0.5f * b; return TapWeights{ wt, wt, wb, wb }; }
CHV_DEV float mix4(float w00, float w10, float w01, float w11, float t00, float t10, float t01, float t11) {
    return ((w00 * t00 + w10 * t10) + w01 * t01) + w11 * t11;      // lin_mix's order (OpenCL 1.2 section 8.2)
}
CHV_DEV float mix4(const TapWeights &w, float t00, float t10, float t01, float t11) { return mix4(w.w00, w.w10, w.w01, w.w11, t00, t10, t01, t11); }
CHV_DEV float cs_mix(const TapWeights &w, float t00, float t10, float t01, float t11) { return cs_mix(w.w00, w.w10, w.w01, w.w11, t00, t10, t01, t11); }

// ---- RGB rows ---------------------------------------------------------------------------------------------------------------------
// Two neighbouring texels (tap columns 0 and 1 of one source row), R, G, B, A whatever the source order
struct TexelPair { float r0, g0, b0, a0, r1, g1, b1, a1; };
// (a pair KEPT from one row to the next lives in eight plain floats at its site: as an aggregate it becomes registers at another point of
// the compilation, and hipcc then numbers the loop's registers differently)
// on the unit scale (c / 255: the reference's float rows)
CHV_DEV TexelPair texels_unit(uint32_t w0, uint32_t w1) {
    return TexelPair{ T8k<0>(w0), T8k<1>(w0), T8k<2>(w0), T8k<3>(w0), T8k<0>(w1), T8k<1>(w1), T8k<2>(w1), T8k<3>(w1) };
}
// on the code scale (the integer-matrix kind).  SWZ: the words are in B, G, R, A order — which byte a conversion reads is free (callers that
// cannot know at compile time put a v_perm_b32 in front)
template <bool SWZ = false>
CHV_DEV TexelPair texels_code(uint32_t w0, uint32_t w1) {
    return TexelPair{ SWZ ? ub2(w0) : ub0(w0), ub1(w0), SWZ ? ub0(w0) : ub2(w0), ub3(w0), SWZ ? ub2(w1) : ub0(w1), ub1(w1), SWZ ? ub0(w1) : ub2(w1), ub3(w1) };
}

// The integer-matrix pixel (img_*_int; statement of record: yuv_pixel.hip.h::apply_yuv_from_rgb_int): the bilinear sample with
// fused multiply-adds on the code scale, rounded to codes; alpha x opacity (ka = opacity / 255)
struct IntPixel { int cr, cg, cb; float a2, ia2; };       // (cr, cg, cb: code_biased's raw bits, what r2y_base_biased expects)
CHV_DEV IntPixel rgb_int_pixel(const TapWeights &w, const TexelPair &t, const TexelPair &b, float ka) {
    const float q0 = cs_mix(w, t.r0, t.r1, b.r0, b.r1);
    const float q1 = cs_mix(w, t.g0, t.g1, b.g0, b.g1);
    const float q2 = cs_mix(w, t.b0, t.b1, b.b0, b.b1);
    const float q3 = cs_mix(w, t.a0, t.a1, b.a0, b.a1);
    // to_code_raw of a convex combination of codes: no clamp can trigger; rint through the float adder (bias kept: r2y_base_biased)
    IntPixel p;
    p.cr = (int)code_biased(q0); p.cg = (int)code_biased(q1); p.cb = (int)code_biased(q2);
    p.a2 = q3 * ka; p.ia2 = 1.f - p.a2;
    return p;
}
// its luma / Cb / Cr code (a float) through the 16.16 matrix
CHV_DEV float r2y_luma(const R2Y &k, const IntPixel &p) {
    return fixed_to_codef(r2y_row(k.y[0], k.y[1], k.y[2], r2y_base_biased(k.y[0], k.y[1], k.y[2], (k.yoff << 16) + 32768), p.cr, p.cg, p.cb));
}
CHV_DEV float r2y_cb(const R2Y &k, const IntPixel &p) {
    return fixed_to_codef(r2y_row(k.u[0], k.u[1], k.u[2], r2y_base_biased(k.u[0], k.u[1], k.u[2], (128 << 16) + 32768), p.cr, p.cg, p.cb));
}
CHV_DEV float r2y_cr(const R2Y &k, const IntPixel &p) {
    return fixed_to_codef(r2y_row(k.v[0], k.v[1], k.v[2], r2y_base_biased(k.v[0], k.v[1], k.v[2], (128 << 16) + 32768), p.cr, p.cg, p.cb));
}

// The float pixel (kernels.cl.swift:509-529): sample, alpha x opacity, rgb2yuv of the pre-multiplied pixel
struct YuvPixel { float yy, uu, vv, a2, ia2; };
CHV_DEV YuvPixel rgb_float_pixel(const TapWeights &w, const TexelPair &t, const TexelPair &b, float opacity) {
    const float r = mix4(w, t.r0, t.r1, b.r0, b.r1);
    const float g = mix4(w, t.g0, t.g1, b.g0, b.g1);
    const float bl = mix4(w, t.b0, t.b1, b.b0, b.b1);
    const float q3 = mix4(w, t.a0, t.a1, b.a0, b.a1);
    YuvPixel p;
    p.a2 = q3 * opacity; p.ia2 = 1.f - p.a2;
    rgb2yuv(r * p.a2, g * p.a2, bl * p.a2, p.yy, p.uu, p.vv);
    return p;
}

// A quad's chroma comes from the even lane's pixel of its even row (the reference's `handleChroma` owner, kernels.cl.swift:76); the lane
// that HOLDS the chroma row is the even lane (even chroma rows) or its odd neighbour (`odd`: u, v, a2, ia2 travel one lane up, in place, and
// with them `take`: the pixel takes the row's result and owns a quad).  Returns the flag that arrived: the holder blends if it is set.
// EVERY: every quad of the strip takes (no flag travels).
template <bool EVERY = false>
CHV_DEV bool quad_chroma(float &u, float &v, float &a2, float &ia2, bool take, bool odd) {
    int stk = take ? 1 : 0;
    if (odd) {
        u = quad_even(u); v = quad_even(v); a2 = quad_even(a2); ia2 = quad_even(ia2);
        if (!EVERY) stk = quad_even(stk);
    }
    return EVERY || stk != 0;
}

// ---- YUV rows (kernels.cl.swift:78-94): cur * (1 - opacity) + sample * opacity --------------------------------------------------------
// A sample at native resolution: the lower tap row of a pixel (b0, b1) is the upper one of the pixel below — its two conversions (three
// instructions each) are carried down the lane in t0, t1.  (Any other sample is mix4 of its four converted taps.)
CHV_DEV float mix4_carried(float &t0, float &t1, float b0, float b1, const TapWeights &w) {
    const float v = mix4(w, t0, t1, b0, b1);
    t0 = b0; t1 = b1;
    return v;
}
// the sample into byte K of a code word.  opaque (opacity == 1): cur * 0 + sample * 1 = sample exactly
template <int K>
CHV_DEV uint32_t yuv_store(uint32_t w, float sample, bool opaque, float alpha, float ialpha) {
    return put_code<K>(w, opaque ? sample : T8k<K>(w) * ialpha + sample * alpha);
}

}  // namespace chv
