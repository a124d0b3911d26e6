// lanczos_to_420_body.hip.h — the row code of the planar Lanczos-3 resampler for the source packings lanczos_420_body.hip.h cannot express
// (DESIGN.md section 4.4.9), for kernels_lanczos_to_420.hip.cpp (chv_scale_lanczos_to_420, chv_scale_lanczos_to_420_ladder).  The arithmetic
// is that of lanczos_planar_body.hip.h, logical image by logical image, so the bytes are.  Luma and planar chroma ARE planar_strip<T, 1>,
// two planar chroma planes into a CbCr plane ARE x420_strip<T, true>, one component of a 2-component plane into a 1-component plane (NV21's
// chroma into y420p, the Y of yuvs / zvuy) IS x420_strip<T, false>.  What is here is chroma read from ONE interleaved plane at a byte offset
// per target component:
//
//   to420_strip<T, 2, 2>   NV21 -> NV12.  The target is the CbCr plane; even lanes (Cb) read byte 1 of the source's texels, odd lanes (Cr) byte 0.
//   to420_strip<T, 4, 1>   yuvs / zvuy -> one chroma plane of y420p.  A chroma texel is four bytes of the packed row (two pixels); the taps are
//                          four bytes apart from byte `off0` (yuvs: Cb 1, Cr 3; zvuy: Cb 0, Cr 2).
//   to420_strip<T, 4, 2>   yuvs / zvuy -> NV12's CbCr plane.  Even lanes start at `off0` (Cb), odd lanes at `off1` (Cr).
//
// The tile route needs nothing new: x420_tile takes a start pointer per component and a tap stride.
#pragma once
#include "lanczos_420_body.hip.h"

#pragma clang fp contract(off)

namespace chv {

// One strip of one chroma target plane of OC components, fed from one plane whose texels are SC bytes: g.src has the LOGICAL image's size
// (texels of SC bytes), the plane's start and pitch.  Everything not commented here is planar_strip<T, C>'s, line by line.
template <int T, int SC, int OC>
CHV_DEV void to420_strip(const PlanarPlane &g, int off0, int off1, int strip, int chunk, int rows_per_wave, uint8_t *lsm) {
    static_assert((SC == 2 || SC == 4) && (OC == 1 || OC == 2), "tap stride 2 or 4 bytes, 1 or 2 target components");
    constexpr int ND = PlanarReads<T, SC>::ND, NA = ND - 1;        // (SC == 4: ND == T, one dword per tap, no realignment)
    const DPlane dst = g.dst, src = g.src;
    const int32_t *__restrict__ fx = g.fx; const float *__restrict__ wx = g.wx;
    const int32_t *__restrict__ fy = g.fy; const float *__restrict__ wy = g.wy;
    const int tx = g.tx, ty = g.ty, nv = g.nv;
    const int lane = threadIdx.x;
    const int wb = dst.w * OC, sb = src.w * SC;
    const int ox0 = strip * 64, j0 = chunk * rows_per_wave;
    if (ox0 >= wb || j0 >= dst.h) return;
    const int nrows = min(rows_per_wave, dst.h - j0);
    const int xb = ox0 + lane, xe = min(xb, wb - 1);
    const int xt = OC == 2 ? xe >> 1 : xe;
    const int off = OC == 2 && (xe & 1) ? off1 : off0;             // this lane's byte within a source texel
    const int b0 = cld<int32_t>((uint64_t)(uintptr_t)(fx + ox0 / OC)) * SC;
    const int b0a = b0 & ~15;
    const int cbyte = gld<int32_t>(fx + xt) * SC - b0a + off;      // tap 0 of this lane, in bytes from the start of the staged row
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
            const int bi = vb + i;                                 // CLAMP_TO_EDGE on the texel index, the byte within the texel kept
            const int ci = SC == 4 ? 4 * min(max(bi >> 2, 0), src.w - 1) + (bi & 3) : 2 * min(max(bi >> 1, 0), src.w - 1) + (bi & 1);
            const uint32_t byte = (uint32_t)gld_at<uint8_t>(rowp, (uint32_t)ci) << (8 * (i & 3));
            if (i < 4) d0 |= byte; else if (i < 8) d1 |= byte; else if (i < 12) d2 |= byte; else d3 |= byte;
        }
        return chv_u32x4{ d0, d1, d2, d3 };
    };
    chv_u32x4 *stage = (chv_u32x4 *)(lsm + planar_wtab_bytes(rows_per_wave, T));      // [2][nv]
    const uint32_t tap0 = (uint32_t)cbyte & ~3u, sh = (uint32_t)cbyte & 3u;
    const int pad = T - ty;
    const int S = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0 + nrows - 1)) - row0 + ty;
    const bool st_vec = ((((uintptr_t)dst.ptr) | (uint32_t)dst.pitch) & 3) == 0;
    const bool st_quad = st_vec && (xb | 3) < wb;
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
    // FAST: as planar_strip.  A lane outside the row replicates its edge TEXEL: two bytes of an NV21 row, the whole dword of a packed one
    // (its Y bytes ride along; no chroma lane reads them).
    const bool fast = vec_ok && sb >= 16 && (sb & 15) == 0;
    const bool edge = b0a < 0 || b0a + 16 * nv > sb;
    const int vbc = min(max(vb, 0), sb - 16);
    auto fix = [&](chv_u32x4 v) -> chv_u32x4 {
        if (vb == vbc) return v;
        const uint32_t rep = vb < 0 ? (SC == 4 ? v.x : (v.x & 0xffffu) * 0x00010001u) : (SC == 4 ? v.w : (v.w >> 16) * 0x00010001u);
        return chv_u32x4{ rep, rep, rep, rep };
    };
    auto rows = [&](auto fastc) {
    constexpr bool FAST = decltype(fastc)::value;
    constexpr int PRE = FAST ? PlanarPre<T>::value : PS_PRE;
#define T4_ISSUE(SLOT, S) do { const int sy_ = min(max(row0 + (S), 0), src.h - 1); \
                               const uint8_t *p_ = src.ptr + (size_t)sy_ * src.pitch + vbc; \
                               asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(SLOT) : "v"(p_) : "memory"); } while (0)
    chv_u32x4 pre[PRE];
#pragma unroll
    for (int p = 0; p < PRE; p++) pre[p] = chv_u32x4{ 0u, 0u, 0u, 0u };
    if (loader) {
#pragma unroll
        for (int p = 0; p < PRE; p++) { if constexpr (FAST) T4_ISSUE(pre[p], p); else pre[p] = load_row(p); }
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
                    T4_ISSUE(pre[t % PRE], s + PRE);
                } else {
                    stage[(t & 1) * nv + lane] = pre[t % PRE];
                    pre[t % PRE] = load_row(s + PRE);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            const uint32_t *row = (const uint32_t *)((const uint8_t *)(stage + (t & 1) * nv) + tap0);
            uint32_t raw[ND];
#pragma unroll
            for (int i = 0; i < ND; i++) raw[i] = row[i];
            float acc = 0.f;
            if constexpr (SC == 4) {                               // tap k is byte sh of dword k
#pragma unroll
                for (int k = 0; k < T; k++) acc = __builtin_fmaf(wr[k], (float)((raw[k] >> (8 * sh)) & 255u), acc);
            } else {
                uint32_t al[NA];
#pragma unroll
                for (int i = 0; i < NA; i++) al[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], sh);
#pragma unroll
                for (int k = 0; k < T; k++) acc = __builtin_fmaf(wr[k], (float)((al[k >> 1] >> (16 * (k & 1))) & 255u), acc);
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
                uint32_t w = 0;
                asm("v_cvt_pk_u8_f32 %0, %1, %2, %0" : "+v"(w) : "v"(o), "v"(lane & 3));
                uint8_t *orow = dst.ptr + (size_t)(j0 + jcur) * dst.pitch;
                if (st_vec) {
                    uint32_t q = w | (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0xB1, 0xF, 0xF, false);     // quad_perm [1, 0, 3, 2]
                    q |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)q, 0x4E, 0xF, 0xF, false);                  // quad_perm [2, 3, 0, 1]
                    if (st_quad) { if ((lane & 3) == 0) gst<uint32_t>(orow + xb, q); }
                    else if (xb < wb) gst<uint8_t>(orow + xb, (uint8_t)(w >> (8 * (lane & 3))));
                } else if (xb < wb) {
                    gst<uint8_t>(orow + xb, (uint8_t)(w >> (8 * (lane & 3))));
                }
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
#undef T4_ISSUE
    };
    if (fast) rows(std::true_type{}); else rows(std::false_type{});
}

}  // namespace chv
