// lanczos_to_yuv_body.hip.h — the row code of the Lanczos-to-YUV kernels (DESIGN.md sections 4.4.2 and 6), shared by the units that launch it:
// kernels_lanczos_to_yuv.hip.cpp (one geometry per launch: lanczos_yuv_strip<T>, lanczos_yuv_tile) and kernels_lanczos_ladder.hip.cpp (all rungs
// of a ladder per launch: lanczos_yuv_ladder<MAXT>, lanczos_yuv_ladder_tile).  The bodies are CHV_DEV templates: they take the picture's planes,
// the block's position inside its picture and the geometry's tables and launch numbers; the kernels around them only find those.  The matrix and
// the target's plane count are read from `a` (any argument struct with the fields n_dst, ybase, ky0 .. kv2), the geometry from `g` (any record
// with the fields fx, wx, fy, wy and nv, rows for the strip body, tx, ty, tw, max_rows for the tile body) where the rows need them.
//
// The host half — which route a geometry takes and with which launch numbers — is here as well, so that both units decide alike.
#pragma once
#include "lanczos_strip_parts.hip.h"
#include "lanczos_route.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace chv {

struct ToYuvArgs {
    const int32_t *fx; const float *wx;
    const int32_t *fy; const float *wy;
    DPlane y, c0, c1, src;            // picture 0's (a batch reads its own from the descriptor list); NV12: c1 is unused
    const DPlane *batch;
    int32_t tx, ty, n_dst;
    int32_t rows, strips, chunks, nv; // strip kernel: output rows per wave (even), blocks along x and y, vectors of a staged row
    int32_t tw, max_rows;             // tile kernel: tile width (32 or 8), rows of the LDS array
    int32_t per_picture, total;       // blocks per picture, blocks in all
    int32_t ybase, ky0, ky1, ky2, ku0, ku1, ku2, kv0, kv1, kv2;      // ybase = (yoff << 16) + 32768
};
static_assert(sizeof(ToYuvArgs) <= 1024, "kernel arguments: 4 KB in all");

struct ToYuvPlanes { DPlane y, c0, c1, src; };

// picture `image`'s planes: a lone call's travel in the arguments, a batch's in the descriptor list (scalar loads)
CHV_DEV ToYuvPlanes yuv_planes(const ToYuvArgs &a, int image) {
    ToYuvPlanes p{ a.y, a.c0, a.c1, a.src };
    if (a.batch) {
        const uint64_t at = (uint64_t)(uintptr_t)a.batch + (uint64_t)image * (a.n_dst + 1) * sizeof(DPlane);
        p.y = cld<DPlane>(at);
        p.c0 = cld<DPlane>(at + sizeof(DPlane));
        p.c1 = cld<DPlane>(at + (a.n_dst == 3 ? 2 : 1) * sizeof(DPlane));
        p.src = cld<DPlane>(at + (uint64_t)a.n_dst * sizeof(DPlane));
    }
    return p;
}

constexpr int32_t kChromaBase = (128 << 16) + 32768;
CHV_DEV uint32_t quad_xor1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false); }      // quad_perm [1, 0, 3, 2]
CHV_DEV uint32_t quad_xor2(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false); }      // quad_perm [2, 3, 0, 1]

// The matrix as the epilogue reads it.  IN_VGPRS: the ten coefficients live in vector registers (the 24-bit multiplier takes them from either
// file) — from 18 taps on, the row of vertical weights and the planes leave the scalar file no room for them.
struct ToYuvMat { int32_t ybase, ky0, ky1, ky2, ku0, ku1, ku2, kv0, kv1, kv2; };
CHV_DEV int32_t in_vgpr(int32_t s) { int32_t v; asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(s)); return v; }
template <bool IN_VGPRS, typename A>
CHV_DEV ToYuvMat yuv_matrix(const A &a) {
    if (IN_VGPRS) return ToYuvMat{ in_vgpr(a.ybase), in_vgpr(a.ky0), in_vgpr(a.ky1), in_vgpr(a.ky2), in_vgpr(a.ku0), in_vgpr(a.ku1), in_vgpr(a.ku2),
                                   in_vgpr(a.kv0), in_vgpr(a.kv1), in_vgpr(a.kv2) };
    return ToYuvMat{ a.ybase, a.ky0, a.ky1, a.ky2, a.ku0, a.ku1, a.ku2, a.kv0, a.kv1, a.kv2 };
}
// a per-lane address the compiler keeps in vector registers (IN_VGPRS) instead of a scalar base and a lane offset
template <bool IN_VGPRS>
CHV_DEV uint8_t *lane_address(uint8_t *p) { if (IN_VGPRS) asm("" : "+v"(p)); return p; }

// clip8(sum >> 16) as clamp(sum, 0, 0xFFFFFF) >> 16: saturate first, then shift (pack_bgra_fixed's form, pixel_math.hip.h — for shift-then-clamp
// hipcc 7.2 selects gfx950's v_ashr_pk_u8_i32 for a pair of codes, whose result's upper half is not zero, and ORs it into the quad's dword)
CHV_DEV uint32_t code_of_fixed(int32_t sum16) { return (uint32_t)min(max(sum16, 0), 0xFFFFFF) >> 16; }
// the luma code of packed codes (byte k: channel k)
CHV_DEV uint32_t yuv_luma(const ToYuvMat &a, uint32_t w) {
    return code_of_fixed(r2y_row(a.ky0, a.ky1, a.ky2, a.ybase, (int)(w & 255u), (int)((w >> 8) & 255u), (int)((w >> 16) & 255u)));
}
// Cb | Cr << 8 of the sums of four codes per channel: channels 0 and 2 as the 16-bit halves of `s02`, channel 1 in `s1` (each below 1021)
CHV_DEV uint32_t yuv_chroma(const ToYuvMat &a, uint32_t s02, uint32_t s1) {
    const uint32_t m02 = ((s02 + 0x00020002u) >> 2) & 0x00ff00ffu;       // (the high half's low bits land above the low half's mean: masked off)
    const int m0 = (int)(m02 & 255u), m1 = (int)((s1 + 2u) >> 2), m2 = (int)(m02 >> 16);
    const uint32_t u = code_of_fixed(r2y_row(a.ku0, a.ku1, a.ku2, kChromaBase, m0, m1, m2));
    const uint32_t v = code_of_fixed(r2y_row(a.kv0, a.kv1, a.kv2, kChromaBase, m0, m1, m2));
    return u | (v << 8);
}

// ---------------------------------------------------------------------------------------------------------------------
// The strip body: one WAVE makes strip `strip` (64 output columns) x chunk `chunk` (`rows_per_wave` output rows, even) of picture P, T taps on
// both axes, a staged row of `nv` vectors.  See lanczos3_strip<T> (kernels_lanczos.hip.cpp) for the structure: the loop runs over SOURCE rows, T
// per trip, window indices and prefetch slots static in every copy of the body; the row loads are issued and awaited by hand
// (tools/check_inflight.py), and the loop holds no other vector load: tables of the rows come through the scalar unit.
//
// TIGHT (the ladder kernels, whose scalar file also carries the way to the rung's record): the trip's first source row and the rows left pass
// through an empty asm once per trip, so the compiler cannot fold them with the static row index t into 2 T loop invariants (row0 + t + PRE and
// S - t for every t, which lanczos_yuv_strip<T> keeps in scalar registers of its own); a row's numbers then cost one scalar add each.  Same
// rows, same bytes.
template <int T, bool TIGHT = false, typename A, typename G>
CHV_DEV void lanczos_yuv_strip_body(const A &a, const ToYuvPlanes &P, const G &g, int chunk, int strip) {
    constexpr int PRE = LanczosPre<T>::value;
    constexpr bool LEAN = T >= 18;                                // (scalar registers: see yuv_matrix)
    const DPlane dst = P.y, src = P.src;
    extern __shared__ __attribute__((aligned(16))) uint8_t ly_lsm[];
    chv_u32x4 *stage = (chv_u32x4 *)ly_lsm;                       // [2][nv]
    const int nv = g.nv, rows_per_wave = g.rows;
    const int lane = threadIdx.x;
    const int ox0 = strip * 64, j0 = chunk * rows_per_wave;
    if (ox0 >= dst.w || j0 >= dst.h) return;
    const int nrows = min(rows_per_wave, dst.h - j0);
    const int x = ox0 + lane, xe = min(x, dst.w - 1);
    const uint64_t fxa = (uint64_t)(uintptr_t)g.fx, fya = (uint64_t)(uintptr_t)g.fy, wya = (uint64_t)(uintptr_t)g.wy;
    const int col0 = cld<int32_t>(fxa + (uint64_t)ox0 * 4);
    const int col0a = col0 & ~3;                                  // (rounds towards -inf: the staged row starts on a 16-byte vector)
    const int cb = gld<int32_t>(g.fx + xe) - col0a;               // tap 0 of this lane, in texels from the start of the staged row
    float wr[T];
#pragma unroll
    for (int k = 0; k < T; k++) wr[k] = gld<float>(g.wx + (size_t)xe * T + k);
    const int row0 = cld<int32_t>(fya + (uint64_t)j0 * 4);
    const bool edge = col0a < 0 || col0a + 4 * nv > src.w;        // (uniform) some staged vector sticks out of the picture
    const int vc = col0a + 4 * lane, vcc = min(max(vc, 0), src.w - 4);
    const bool loader = lane < nv;
    auto fix = [&](chv_u32x4 L) {                                  // texel k of the vector = texel clamp(vc + k) of the row
        auto pick = [&](int k) {
            const int i2 = min(max(vc + k, 0), src.w - 1) - vcc;
            return i2 == 0 ? L.x : i2 == 1 ? L.y : i2 == 2 ? L.z : L.w;
        };
        chv_u32x4 r = { pick(0), pick(1), pick(2), pick(3) };
        return r;
    };
    // (the asm names the prefetch slot itself as its output: no temporary the compiler could copy from before the data has landed)
#define LY_ISSUE(SLOT, ROW) do { const int sy_ = min(max((ROW), 0), src.h - 1); \
                               const uint8_t *p_ = src.ptr + (size_t)sy_ * src.pitch + (size_t)vcc * 4; \
                               asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(SLOT) : "v"(p_) : "memory"); } while (0)
    chv_u32x4 pre[PRE];
#pragma unroll
    for (int p = 0; p < PRE; p++) pre[p] = chv_u32x4{ 0u, 0u, 0u, 0u };
    if (loader) {
#pragma unroll
        for (int p = 0; p < PRE; p++) LY_ISSUE(pre[p], row0 + (p));
    }
    float h0[T], h1[T], h2[T];
#pragma unroll
    for (int t = 0; t < T; t++) { h0[t] = 0.f; h1[t] = 0.f; h2[t] = 0.f; }
    const uint32_t tap0 = (uint32_t)cb * 4u;
    const int S = cld<int32_t>(fya + (uint64_t)(j0 + nrows - 1) * 4) - row0 + T;       // source rows this strip filters
    // where the rows go.  Luma: a dword per quad wherever the plane's start and pitch are 4-byte aligned (uniform) and the quad lies inside
    // the row.  Chroma: the even lane of a column pair owns texel x / 2 — NV12 pairs of a quad leave as one dword under the same conditions.
    const int cw = P.c0.w, chh = P.c0.h;
    const bool nv12 = a.n_dst == 2;
    const bool st_vec = ((((uintptr_t)dst.ptr) | (uint32_t)dst.pitch) & 3) == 0;
    const bool st_quad = st_vec && (x | 3) < dst.w;
    const bool c_vec = nv12 && ((((uintptr_t)P.c0.ptr) | (uint32_t)P.c0.pitch) & 3) == 0;
    const int cx = x >> 1;
    const bool c_own = (lane & 1) == 0 && cx < cw;
    const bool c_quad = c_vec && (cx | 1) < cw;
    const uint32_t ysh = 8u * (uint32_t)(lane & 3);
    const ToYuvMat mat = yuv_matrix<LEAN>(a);
    uint8_t *const ycol = lane_address<LEAN>(dst.ptr + x);        // this lane's byte of luma row 0; its chroma texel of chroma row 0
    uint8_t *const c0col = lane_address<LEAN>(P.c0.ptr + (nv12 ? 2 * cx : cx)), *const c1col = lane_address<LEAN>(P.c1.ptr + cx);
    auto chroma_row = [&](uint32_t even, uint32_t odd, int cy) {  // (all lanes: the sums cross the pair through DPP)
        uint32_t s02 = (even & 0x00ff00ffu) + (odd & 0x00ff00ffu), s1 = ((even >> 8) & 255u) + ((odd >> 8) & 255u);
        s02 += quad_xor1(s02); s1 += quad_xor1(s1);
        const uint32_t uv = yuv_chroma(mat, s02, s1);
        const uint32_t uv2 = uv | (quad_xor2(uv) << 16);          // lane 4 q: texels 2 q and 2 q + 1
        if (cy >= chh) return;                                    // (uniform)
        uint8_t *c0p = c0col + (size_t)cy * P.c0.pitch;
        if (nv12) {
            if (c_quad) { if ((lane & 3) == 0) gst<uint32_t>(c0p, uv2); }
            else if (c_own) { gst<uint8_t>(c0p, (uint8_t)uv); gst<uint8_t>(c0p + 1, (uint8_t)(uv >> 8)); }
        } else if (c_own) {
            gst<uint8_t>(c0p, (uint8_t)uv);
            gst<uint8_t>(c1col + (size_t)cy * P.c1.pitch, (uint8_t)(uv >> 8));
        }
    };
    uint32_t even_codes = 0;                                      // the packed codes of the chunk's last even row
    int jcur = 0, fcur = 0;                                       // next output row to finish, its first source row (fy[j0] - row0 = 0)
    for (int gi = 0; gi * T < S; gi++) {
        // A source row has three numbers, each written in two forms that an edit must keep in step.  With s = trip + t (t static, trip = gi * T):
        //   past the last row:        s >= S              <=>  t >= left                    (left = S - trip)
        //   the row to prefetch:      row0 + (s + PRE)     ==  trip_row + (t + PRE)         (trip_row = row0 + trip)
        //   an output row ends here:  fcur + T - 1 == s   <=>  fcur + (T - 1 - t) == trip
        // The left forms are lanczos_yuv_strip<T>'s (trip, trip_row and left are dead there); the right forms are TIGHT's.
        int trip = gi * T, trip_row = row0 + trip, left = S - trip;
        if (TIGHT) asm("" : "+s"(trip), "+s"(trip_row), "+s"(left));
        auto body = [&](auto tc) -> bool {
            constexpr int t = decltype(tc)::value;
            const int s = gi * T + t;
            if (TIGHT ? t >= left : s >= S) return false;         // (uniform)
            if (loader) {
                asm volatile("s_waitcnt vmcnt(%1)" : "+v"(pre[t % PRE]) : "n"(PRE - 1) : "memory");
                stage[(t & 1) * nv + lane] = edge ? fix(pre[t % PRE]) : pre[t % PRE];
                LY_ISSUE(pre[t % PRE], TIGHT ? trip_row + (t + PRE) : row0 + (s + PRE));
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            const uint32_t *row = (const uint32_t *)((const uint8_t *)(stage + (t & 1) * nv) + tap0);
            uint32_t e[T];
#pragma unroll
            for (int k = 0; k < T; k++) e[k] = row[k];
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int k = 0; k < T; k++) {
                a0 = __builtin_fmaf(wr[k], (float)(e[k] & 255), a0);
                a1 = __builtin_fmaf(wr[k], (float)((e[k] >> 8) & 255), a1);
                a2 = __builtin_fmaf(wr[k], (float)((e[k] >> 16) & 255), a2);
            }
            h0[t] = a0; h1[t] = a1; h2[t] = a2;
            // output rows whose last source row this was: source rows s - T + 1 .. s are window rows (t + 1) % T, (t + 2) % T, ...
            while (jcur < nrows && (TIGHT ? fcur + (T - 1 - t) == trip : fcur + T - 1 == s)) {           // (uniform; at most once per source row when reducing)
                const int oy = j0 + jcur;
                const uint64_t wrow = wya + (uint64_t)oy * T * 4;
                float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
                for (int k = 0; k < T; k++) {
                    const float wk = cld<float>(wrow + 4 * k);
                    o0 = __builtin_fmaf(wk, h0[(t + 1 + k) % T], o0);
                    o1 = __builtin_fmaf(wk, h1[(t + 1 + k) % T], o1);
                    o2 = __builtin_fmaf(wk, h2[(t + 1 + k) % T], o2);
                }
                const uint32_t codes = pack_codes(o0, o1, o2, 0u);
                const uint32_t yb = yuv_luma(mat, codes) << ysh;
                uint8_t *yp = ycol + (size_t)oy * dst.pitch;
                if (st_vec) {
                    uint32_t q = yb | quad_xor1(yb);
                    q |= quad_xor2(q);
                    if (st_quad) { if ((lane & 3) == 0) gst<uint32_t>(yp, q); }
                    else if (x < dst.w) gst<uint8_t>(yp, (uint8_t)(yb >> ysh));           // the row's last, partial quad
                } else if (x < dst.w) {
                    gst<uint8_t>(yp, (uint8_t)(yb >> ysh));
                }
                if (oy & 1) chroma_row(even_codes, codes, oy >> 1);
                else {
                    even_codes = codes;
                    if (oy == dst.h - 1) chroma_row(codes, codes, oy >> 1);      // a 1-high picture: the clamped quad (an odd height's last row
                }                                                               // has no chroma row: chroma_row returns)
                jcur++;
                if (jcur < nrows) fcur = cld<int32_t>(fya + (uint64_t)(j0 + jcur) * 4) - row0;
            }
            return true;
        };
        lanczos_all_of(body, std::make_integer_sequence<int, T>{});
    }
#pragma unroll
    for (int p = 0; p < PRE; p++) asm volatile("s_waitcnt vmcnt(0)" : "+v"(pre[p]) :: "memory");
#undef LY_ISSUE
}

// ---------------------------------------------------------------------------------------------------------------------
// The tile body — any tap counts.  A block of 256 threads makes tile (bx, by) of tw x 4 output pixels: the horizontal pass reads its taps from
// global memory (CLAMP_TO_EDGE on the texel index) and leaves three floats per (source row, column) in LDS; the vertical pass runs out of it
// with lanes 4 q .. 4 q + 3 on the 2 x 2 pixels of chroma texel q (tile sizes are even: a quad never spans tiles), so the box sum is two DPP
// adds.  Pixels beyond the picture's last column or row are computed at the clamped position — the clamped quad of section 4.4.2 — and not stored.
constexpr int YT_H = 4;

template <typename A, typename G>
CHV_DEV void lanczos_yuv_tile_body(const A &a, const ToYuvPlanes &P, const G &g, int by, int bx) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ly_lsm[];
    float *hrow = (float *)ly_lsm;                                 // [max_rows][tw][3]
    const DPlane dst = P.y, src = P.src;
    const int tx = g.tx, ty = g.ty, tw = g.tw;
    const int ox0 = bx * tw, oy0 = by * YT_H;
    if (ox0 >= dst.w || oy0 >= dst.h) return;
    const int oy_last = min(oy0 + YT_H, dst.h) - 1;
    const int row0 = gld<int32_t>(g.fy + oy0);
    const int nrows = min(gld<int32_t>(g.fy + oy_last) + ty - row0, g.max_rows);
    const int tid = threadIdx.x;
    const ToYuvMat mat = yuv_matrix<false>(a);
    for (int e = tid; e < nrows * tw; e += 256) {
        const int r = e / tw, i = e - r * tw;
        const int xe = min(ox0 + i, dst.w - 1);
        const int f = gld<int32_t>(g.fx + xe);
        const float *w = g.wx + (size_t)xe * tx;
        const uint8_t *rowp = src.ptr + (size_t)min(max(row0 + r, 0), src.h - 1) * src.pitch;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < tx; k++) {
            const uint32_t p = gld<uint32_t>(rowp + (size_t)min(max(f + k, 0), src.w - 1) * 4);
            const float wk = gld<float>(w + k);
            a0 = __builtin_fmaf(wk, (float)(p & 255), a0);
            a1 = __builtin_fmaf(wk, (float)((p >> 8) & 255), a1);
            a2 = __builtin_fmaf(wk, (float)((p >> 16) & 255), a2);
        }
        hrow[3 * e] = a0; hrow[3 * e + 1] = a1; hrow[3 * e + 2] = a2;
    }
    __syncthreads();
    if (tid < tw * YT_H) {                                         // (whole quads: tw * 4 is a multiple of 4)
        const int q = tid >> 2, qy = q / (tw >> 1), qx = q - qy * (tw >> 1);
        const int i = 2 * qx + (tid & 1), j = 2 * qy + ((tid >> 1) & 1);
        const int x = ox0 + i, oy = oy0 + j, oye = min(oy, dst.h - 1);
        const int rbase = gld<int32_t>(g.fy + oye) - row0;
        const float *w = g.wy + (size_t)oye * ty;
        float o0 = 0.f, o1 = 0.f, o2 = 0.f;
        for (int k = 0; k < ty; k++) {
            const float wk = gld<float>(w + k);
            const float *hp = hrow + 3 * ((rbase + k) * tw + i);
            o0 = __builtin_fmaf(wk, hp[0], o0);
            o1 = __builtin_fmaf(wk, hp[1], o1);
            o2 = __builtin_fmaf(wk, hp[2], o2);
        }
        const uint32_t codes = pack_codes(o0, o1, o2, 0u);
        if (x < dst.w && oy < dst.h) gst<uint8_t>(dst.ptr + (size_t)oy * dst.pitch + x, (uint8_t)yuv_luma(mat, codes));
        uint32_t s02 = codes & 0x00ff00ffu, s1 = (codes >> 8) & 255u;
        s02 += quad_xor1(s02); s1 += quad_xor1(s1);
        s02 += quad_xor2(s02); s1 += quad_xor2(s1);
        const uint32_t uv = yuv_chroma(mat, s02, s1);
        const int cx = x >> 1, cy = oy >> 1;
        if ((tid & 3) == 0 && cx < P.c0.w && cy < P.c0.h) {
            if (a.n_dst == 2) {
                uint8_t *cp = P.c0.ptr + (size_t)cy * P.c0.pitch + 2 * cx;
                gst<uint8_t>(cp, (uint8_t)uv); gst<uint8_t>(cp + 1, (uint8_t)(uv >> 8));
            } else {
                gst<uint8_t>(P.c0.ptr + (size_t)cy * P.c0.pitch + cx, (uint8_t)uv);
                gst<uint8_t>(P.c1.ptr + (size_t)cy * P.c1.pitch + cx, (uint8_t)(uv >> 8));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The host half: the route of one geometry.

// (the refusal is chv_scale_lanczos's for the same geometry: lanczos_refuses, lanczos_route.h)

// The wave-per-strip kernel takes equal, even tap counts 6 .. 22 on both axes, a source of at least 4 texels and a staged row of at most 64
// vectors: the vectors of that row, 0 for every other geometry (the tile kernel's).
inline int to_yuv_strip_vectors(int dw, int sw, int tx, int ty) {
    if (!(tx == ty && tx <= 22 && (tx & 1) == 0 && tx >= 6 && sw >= 4)) return 0;
    const double sxs = (double)sw / (double)dw;
    const int nv = ((int)(63 * sxs) + 1 + 3 + tx + 3) / 4 + 1;          // fx[x + 63] - fx[x] <= floor(63 scale) + 1; 3 texels of alignment
    return nv <= 64 ? nv : 0;
}

// rows per wave of the strip kernel for `work` = the launch's output rows x strips x pictures, as launch_lanczos chooses them — and even: a
// chunk starts on an even output row, its chroma rows are its own
inline int to_yuv_strip_rows(long work) { return (lanczos_strip_rows(work, 256) + 1) & ~1; }

// the tile kernel: 32 x 4 pixels while the horizontally filtered rows of a tile fit 48 KB of LDS, 8 x 4 beyond (at most 256 taps and the
// refusal above bound the 8-wide array by 37 KB).  Returns the dynamic LDS in bytes.
inline size_t to_yuv_tile_shape(int dh, int sh, int ty, int *tw, int *max_rows) {
    const double sy = (double)sh / (double)dh;
    *max_rows = (int)((YT_H - 1) * sy + 2) + ty;
    *tw = (size_t)*max_rows * 32 * 3 * sizeof(float) <= 48 * 1024 ? 32 : 8;
    return (size_t)*max_rows * *tw * 3 * sizeof(float);
}

}  // namespace chv
