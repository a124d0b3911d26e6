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
// The host half — THE routing rule of these entries — is at the end.
#pragma once
#include "lanczos_planar_body.hip.h"

#pragma clang fp contract(off)

namespace chv {

// One strip of one chroma target plane.  g.src: the CbCr plane (NV12 source) or the Cb plane (y420p source), src2: the Cr plane of a y420p
// source (same width and height as Cb; its own start and pitch).  Everything not commented here is planar_strip<T, C>'s, line by line.
template <int T, bool TO_NV12>
CHV_DEV void x420_strip(const PlanarPlane &g, const DPlane &src2, int comp_in, int strip, int chunk, int rows_per_wave, uint8_t *lsm) {
    constexpr int OC = TO_NV12 ? 2 : 1, SC = TO_NV12 ? 1 : 2;      // components of a target texel, of a source texel: the tap stride
    constexpr int ND = PlanarReads<T, SC>::ND, NA = ND - 1;
    const DPlane dst = g.dst, src = g.src;
    const int32_t *__restrict__ fx = g.fx; const float *__restrict__ wx = g.wx;
    const int32_t *__restrict__ fy = g.fy; const float *__restrict__ wy = g.wy;
    const int tx = g.tx, ty = g.ty, nv = g.nv;                     // nv: vectors of one staged row of ONE source plane
    const int lane = threadIdx.x;
    const int wb = dst.w * OC, sb = src.w * SC;
    const int ox0 = strip * 64, j0 = chunk * rows_per_wave;
    if (ox0 >= wb || j0 >= dst.h) return;
    const int nrows = min(rows_per_wave, dst.h - j0);
    const int xb = ox0 + lane, xe = min(xb, wb - 1);
    const int xt = OC == 2 ? xe >> 1 : xe, comp = OC == 2 ? xe & 1 : comp_in;
    const int b0 = cld<int32_t>((uint64_t)(uintptr_t)(fx + ox0 / OC)) * SC;
    const int b0a = b0 & ~15;
    // tap 0 of this lane, in bytes from the start of the ring slot: a Cr lane of the y420p source reads the slot's second half
    const int ring = TO_NV12 ? 2 * nv : nv;                        // vectors of one ring slot
    const int cbyte = gld<int32_t>(fx + xt) * SC - b0a + (TO_NV12 ? comp * nv * 16 : comp);
    float wr[T];
#pragma unroll
    for (int k = 0; k < T; k++) {
        const float wk = gld<float>(wx + (size_t)xt * tx + min(k, tx - 1));
        wr[k] = k < tx ? wk : 0.f;
    }
    const int row0 = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0));
    // Loader lanes: [0, nv) stage the row of g.src, and for a y420p source [nv, 2 nv) the row of src2.  2 nv <= 64 for every strip-route
    // geometry: at most 22 taps means a scale of at most 11 / 3, so the strip's 32 texel columns span at most 114 source texels, and with 15
    // bytes of alignment and the last column's dword reads nv <= 12.  (x420_strip_route checks it all the same.)
    const bool second = TO_NV12 && lane >= nv;
    const int li = second ? lane - nv : lane;
    const uint8_t *sptr = second ? src2.ptr : src.ptr;
    const int spitch = second ? src2.pitch : src.pitch;
    const bool ok1 = ((((uintptr_t)src.ptr) | (uint32_t)src.pitch) & 3) == 0;
    const bool ok2 = !TO_NV12 || ((((uintptr_t)src2.ptr) | (uint32_t)src2.pitch) & 3) == 0;
    const bool vec_ok = second ? ok2 : ok1;                        // (per lane: a plane at an odd byte is gathered, its sibling need not be)
    const int vb = b0a + 16 * li;
    const bool loader = lane < ring;
    const bool vec_lane = vec_ok && vb >= 0 && vb + 16 <= sb;
    auto load_row = [&](int s) -> chv_u32x4 {
        const int sy = min(max(row0 + s, 0), src.h - 1);
        const uint8_t *rowp = sptr + (size_t)sy * spitch;
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
    chv_u32x4 *stage = (chv_u32x4 *)(lsm + planar_wtab_bytes(rows_per_wave, T));      // [2][ring]
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
    // FAST (uniform per target plane): BOTH source planes of a y420p source must qualify — one wait covers the loads of both halves.  Edge
    // replication is per plane: a lane outside its row loads its OWN plane's first / last vector.
    const bool fast = ok1 && ok2 && sb >= 16 && (sb & 15) == 0;
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
#define X4_ISSUE(SLOT, S) do { const int sy_ = min(max(row0 + (S), 0), src.h - 1); \
                               const uint8_t *p_ = sptr + (size_t)sy_ * spitch + vbc; \
                               asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(SLOT) : "v"(p_) : "memory"); } while (0)
    chv_u32x4 pre[PRE];
#pragma unroll
    for (int p = 0; p < PRE; p++) pre[p] = chv_u32x4{ 0u, 0u, 0u, 0u };
    if (loader) {
#pragma unroll
        for (int p = 0; p < PRE; p++) { if constexpr (FAST) X4_ISSUE(pre[p], p); else pre[p] = load_row(p); }
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
                    stage[(t & 1) * ring + lane] = edge ? fix(pre[t % PRE]) : pre[t % PRE];
                    X4_ISSUE(pre[t % PRE], s + PRE);
                } else {
                    stage[(t & 1) * ring + lane] = pre[t % PRE];
                    pre[t % PRE] = load_row(s + PRE);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            const uint32_t *row = (const uint32_t *)((const uint8_t *)(stage + (t & 1) * ring) + tap0);
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
#undef X4_ISSUE
    };
    if (fast) rows(std::true_type{}); else rows(std::false_type{});
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

// ---------------------------------------------------------------------------------------------------------------------
// THE routing rule of chv_scale_lanczos_420 / _ladder (they read no switch).  `pl`: the np target planes of one rung with dst, src (sizes and
// component counts: src.comps is what the source plane that feeds this target plane has), tx and ty filled in.  Strip route (true): no plane
// has more than 22 taps on an axis and no ring slot is longer than 64 vectors — planar_strip_route's rule with the source's own tap stride:
// a target plane of OC components fed from a plane of SC stages the span of its 64 / OC texel columns in SC bytes per texel, and a CbCr
// target fed from two planes stages one such row of each.  *T: the tap class; every plane's nv (vectors of ONE staged row) is set,
// *ring_max is the longest ring slot.  Tile route otherwise.
inline bool x420_strip_route(PlanarPlane *pl, int np, int *T, int *ring_max) {
    int tmax = 0;
    for (int p = 0; p < np; p++) tmax = std::max(tmax, std::max(pl[p].tx, pl[p].ty));
    *T = tmax <= 6 ? 6 : tmax <= 8 ? 8 : tmax <= 12 ? 12 : tmax <= 16 ? 16 : 22;
    *ring_max = 0;
    if (tmax > 22) return false;
    for (int p = 0; p < np; p++) {
        PlanarPlane &g = pl[p];
        const int OC = g.dst.comps, SC = g.src.comps;
        const double sx = (double)g.src.w / (double)g.dst.w;
        const int span = ((int)((64 / OC - 1) * sx) + 1) * SC + (SC - 1);
        const int bytes = 15 + span + 4 * (((*T * SC - SC + 7) / 4) + 1);
        g.nv = (bytes + 15) / 16 + 1;
        *ring_max = std::max(*ring_max, OC == 2 && SC == 1 ? 2 * g.nv : g.nv);
    }
    return *ring_max <= 64;
}

}  // namespace chv
