// lanczos_from_yuv_body.hip.h — the row code of the Lanczos-3 resampler FROM a 4:2:0 picture INTO a BGRA / RGBA plane (DESIGN.md section
// 4.4.6), for kernels_lanczos_from_yuv.hip.cpp (chv_scale_lanczos_from_yuv, chv_scale_lanczos_from_yuv_batch).  Every logical plane (Y, Cb,
// Cr) is resampled to the TARGET's size by the arithmetic of lanczos_planar_body.hip.h and rounded to a code; the three codes of a pixel go
// through the integer matrix of section 4.2.  Nothing crosses from one plane into another before its code is rounded, so the order in which a
// block resamples its planes is free:
//
//   fy_strip<T, SC>   one strip of one logical plane: 64 output columns x `rows` output rows, the structure of planar_strip<T, 1> /
//                     x420_strip<T, false> line by line — source rows staged through a two-row LDS ring with 16-byte loads (issued and awaited
//                     by hand on vector-aligned planes), a window of T floats in the lane's registers, the vertical weights in LDS.  SC is the
//                     tap stride: 1 for a plane of its own, 2 for component `comp` of an NV12 picture's CbCr plane.  What differs is where a
//                     finished output value goes: to `sink(row, value)`, not to memory.  A wave runs it three times over the same block: Cb
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
// holds the logical plane, of SC components; comp: the component.  Everything not commented here is planar_strip<T, C>'s.
template <int T, int SC, typename Sink>
CHV_DEV void fy_strip(const PlanarPlane &g, int comp, int strip, int chunk, int rows_per_wave, uint8_t *lsm, Sink &&sink) {
    constexpr int ND = PlanarReads<T, SC>::ND, NA = ND - 1;
    const DPlane dst = g.dst, src = g.src;
    const int32_t *__restrict__ fx = g.fx; const float *__restrict__ wx = g.wx;
    const int32_t *__restrict__ fy = g.fy; const float *__restrict__ wy = g.wy;
    const int tx = g.tx, ty = g.ty, nv = g.nv;
    const int lane = threadIdx.x;
    const int wb = dst.w, sb = src.w * SC;
    const int ox0 = strip * 64, j0 = chunk * rows_per_wave;
    if (ox0 >= wb || j0 >= dst.h) return;
    const int nrows = min(rows_per_wave, dst.h - j0);
    const int xt = min(ox0 + lane, wb - 1);
    const int b0 = cld<int32_t>((uint64_t)(uintptr_t)(fx + ox0)) * SC;
    const int b0a = b0 & ~15;
    const int cbyte = gld<int32_t>(fx + xt) * SC - b0a + comp;
    float wr[T];
#pragma unroll
    for (int k = 0; k < T; k++) {
        const float wk = gld<float>(wx + (size_t)xt * tx + min(k, tx - 1));
        wr[k] = k < tx ? wk : 0.f;
    }
    const int row0 = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0));
    const bool vec_ok = ((((uintptr_t)src.ptr) | (uint32_t)src.pitch) & 3) == 0;
    const int vb = b0a + 16 * lane;
    const bool loader = lane < nv;
    const bool vec_lane = vec_ok && vb >= 0 && vb + 16 <= sb;
    auto load_row = [&](int s) -> chv_u32x4 {
        const int sy = min(max(row0 + s, 0), src.h - 1);
        const uint8_t *rowp = src.ptr + (size_t)sy * src.pitch;
        if (vec_lane) return *(const CHV_GLOBAL chv_u32x4 *)(uintptr_t)(rowp + vb);
        uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int bi = vb + i;
            const int ci = SC == 2 ? 2 * min(max(bi >> 1, 0), src.w - 1) + (bi & 1) : min(max(bi, 0), sb - 1);
            const uint32_t byte = (uint32_t)gld_at<uint8_t>(rowp, (uint32_t)ci) << (8 * (i & 3));
            if (i < 4) d0 |= byte; else if (i < 8) d1 |= byte; else if (i < 12) d2 |= byte; else d3 |= byte;
        }
        return chv_u32x4{ d0, d1, d2, d3 };
    };
    chv_u32x4 *stage = (chv_u32x4 *)(lsm + planar_wtab_bytes(rows_per_wave, T));      // [2][nv]
    const uint32_t tap0 = (uint32_t)cbyte & ~3u, sh = (uint32_t)cbyte & 3u;
    const int pad = T - ty;
    const int S = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0 + nrows - 1)) - row0 + ty;
    float *wtab = (float *)lsm;                                    // [nrows][T]
    for (int e0 = lane; e0 < nrows * T; e0 += 64 * 8) {
        float wk[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int e = min(e0 + 64 * u, nrows * T - 1), j = e / T, k = e - j * T;
            wk[u] = gld<float>(wy + (size_t)(j0 + j) * ty + max(k - pad, 0));
            if (k < pad) wk[u] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) if (e0 + 64 * u < nrows * T) wtab[e0 + 64 * u] = wk[u];
    }
    // FAST: planar_strip's condition and planar_strip's hand-awaited row loads (tools/check_inflight.py walks this unit's object too)
    const bool fast = vec_ok && sb >= 16 && (sb & 15) == 0;
    const bool edge = b0a < 0 || b0a + 16 * nv > sb;
    const int vbc = min(max(vb, 0), sb - 16);
    auto fix = [&](chv_u32x4 v) -> chv_u32x4 {
        if (vb == vbc) return v;
        const uint32_t rep = vb < 0 ? (SC == 2 ? (v.x & 0xffffu) * 0x00010001u : (v.x & 255u) * 0x01010101u)
                                    : (SC == 2 ? (v.w >> 16) * 0x00010001u : (v.w >> 24) * 0x01010101u);
        return chv_u32x4{ rep, rep, rep, rep };
    };
    auto rows = [&](auto fastc) {
    constexpr bool FAST = decltype(fastc)::value;
    constexpr int PRE = FAST ? PlanarPre<T>::value : PS_PRE;
#define FY_ISSUE(SLOT, S) do { const int sy_ = min(max(row0 + (S), 0), src.h - 1); \
                               const uint8_t *p_ = src.ptr + (size_t)sy_ * src.pitch + vbc; \
                               asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(SLOT) : "v"(p_) : "memory"); } while (0)
    chv_u32x4 pre[PRE];
#pragma unroll
    for (int p = 0; p < PRE; p++) pre[p] = chv_u32x4{ 0u, 0u, 0u, 0u };
    if (loader) {
#pragma unroll
        for (int p = 0; p < PRE; p++) { if constexpr (FAST) FY_ISSUE(pre[p], p); else pre[p] = load_row(p); }
    }
    float h[T];
#pragma unroll
    for (int t = 0; t < T; t++) h[t] = 0.f;
    int jcur = 0, fcur = 0;
    for (int gi = 0; gi * T < S; gi++) {
        auto body = [&](auto tc) -> bool {
            constexpr int t = decltype(tc)::value;
            const int s = gi * T + t;
            if (s >= S) return false;                              // (uniform)
            if (loader) {
                if constexpr (FAST) {
                    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(pre[t % PRE]) : "n"(PRE - 1) : "memory");
                    stage[(t & 1) * nv + lane] = edge ? fix(pre[t % PRE]) : pre[t % PRE];
                    FY_ISSUE(pre[t % PRE], s + PRE);
                } else {
                    stage[(t & 1) * nv + lane] = pre[t % PRE];
                    pre[t % PRE] = load_row(s + PRE);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            const uint32_t *row = (const uint32_t *)((const uint8_t *)(stage + (t & 1) * nv) + tap0);
            uint32_t raw[ND], al[NA];
#pragma unroll
            for (int i = 0; i < ND; i++) raw[i] = row[i];
#pragma unroll
            for (int i = 0; i < NA; i++) al[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], sh);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < T; k++) {
                const uint32_t word = SC == 2 ? al[k >> 1] : al[k >> 2];
                const uint32_t byte = SC == 2 ? (word >> (16 * (k & 1))) & 255u : (word >> (8 * (k & 3))) & 255u;
                acc = __builtin_fmaf(wr[k], (float)byte, acc);
            }
            h[t] = acc;
            while (jcur < nrows && fcur + ty - 1 == s) {           // (uniform)
                const float2 *wrow = (const float2 *)(wtab + jcur * T);
                float o = 0.f;
#pragma unroll
                for (int k = 0; k < T; k += 2) {
                    const float2 wk = wrow[k >> 1];
                    o = __builtin_fmaf(wk.x, h[(t + 1 + k) % T], o);
                    o = __builtin_fmaf(wk.y, h[(t + 2 + k) % T], o);
                }
                sink(jcur, o);                                     // the plane's value of (column ox0 + lane, row j0 + jcur), before rounding
                jcur++;
                if (jcur < nrows) fcur = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0 + jcur)) - row0;
            }
            return true;
        };
        planar_all_of(body, std::make_integer_sequence<int, T>{});
    }
    if constexpr (FAST) {
#pragma unroll
        for (int p = 0; p < PRE; p++) asm volatile("s_waitcnt vmcnt(0)" : "+v"(pre[p]) :: "memory");
    }
#undef FY_ISSUE
    };
    if (fast) rows(std::true_type{}); else rows(std::false_type{});
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
    auto cls = [](int t) { return t <= 6 ? 6 : t <= 8 ? 8 : t <= 12 ? 12 : t <= 16 ? 16 : 22; };
    *TL = cls(std::max(pl[0].tx, pl[0].ty));
    *TC = cls(std::max(pl[1].tx, pl[1].ty));
    return *TC <= 12;
}

// rows per wave: planar_strip_rows on the (strip, output row) pairs of the launch, at most FY_MAX_ROWS
inline int fy_strip_rows(long work) { return std::min(planar_strip_rows(work), FY_MAX_ROWS); }

// LDS of one wave on the strip route: the vertical weights of the widest body, the longest ring, the codes of Cb and Cr
inline size_t fy_codes_at(int rows, int TL, int TC, int ring_max) { return planar_wtab_bytes(rows, std::max(TL, TC)) + (size_t)2 * ring_max * 16; }
inline size_t fy_strip_lds(int rows, int TL, int TC, int ring_max) { return fy_codes_at(rows, TL, TC, ring_max) + (size_t)2 * 64 * rows; }

}  // namespace chv
