// lanczos_rgb_body.hip.h — the row code of the 4-component Lanczos-3 LADDER (DESIGN.md sections 4.4 and 4.4.8), launched by
// kernels_lanczos_rgb_ladder.hip.cpp.  The arithmetic is chv_scale_lanczos's on one BGRA / RGBA plane (kernels_lanczos.hip.cpp): per
// component, a horizontal chain and a vertical chain that start at 0.0f and take their taps ascending, one fmaf per tap — so the bytes are.
//
//   rgb_strip<T>   tx, ty <= T <= 22: one WAVE per strip of 64 output columns x `rows` output rows, in the manner of lanczos3_strip<T>: a lane
//                  owns one output column for both passes, source rows staged through a two-row LDS ring with 16-byte loads (issued and
//                  awaited by hand), the horizontal results of the last T source rows in a window of T float4 in the lane's registers, the
//                  strip's vertical weights in LDS, a dword store per lane, no block barrier, no scratch.  Unlike lanczos3_strip<T> the geometry's tap counts need not EQUAL T,
//                  on either axis: lanczos_planar_body.hip.h's padding.
//   rgb_tile       everything else: 256 threads per tile of tw x 4 output pixels (tw 32, or 8 where 32 columns of the rows a tile needs
//                  would not fit 64 KB), horizontal pass from global memory into LDS, vertical pass out of it.  Simple on purpose.
//
// The host half — which route a geometry takes, its launch numbers — is here too, so that the launcher does not restate it.
#pragma once
#include "lanczos_strip_parts.hip.h"
#include "lanczos_route.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace chv {

// what a block needs to know about its rung's geometry (kernel arguments: read through the constant address space at a uniform index, never
// by indexing a private copy of the argument — lanczos_planar_body.hip.h)
struct RgbGeom {
    const int32_t *fx; const float *wx;
    const int32_t *fy; const float *wy;
    int32_t tx, ty;
    int32_t nv;                       // strip route: 16-byte vectors of one staged source row (sized for the rung's T, not for tx)
    int32_t max_rows;                 // tile route: rows of the LDS array
    int32_t tw;                       // tile route: output columns per tile
    int32_t T;                        // strip route: the rung's own tap class (6 / 8 / 12 / 16 / 22 over its larger tap count)
};

constexpr int RS_MAX_ROWS = 64;      // output rows per wave at most: their vertical weights live in LDS

// One strip: 64 output columns, rows [chunk * rows_per_wave, ...).  tx, ty <= T: the taps beyond tx read a staged texel with weight 0 in the
// horizontal pass (fma(0, finite, acc) == acc; the chain starts at +0 and a sum with +0 in it is never -0), and the vertical pass walks the
// whole window with the weights of the rows older than ty set to 0 — window indices stay static whatever the rung's tap counts are.  The
// loop runs over SOURCE rows, T per trip (lanczos3_strip<T> says why); an output row finishes at source row fy[j] + ty - 1.
template <int T>
CHV_DEV void rgb_strip(const RgbGeom &g, const DPlane &dst, const DPlane &src, int strip, int chunk, int rows_per_wave, uint8_t *lsm) {
    constexpr int PRE = LanczosPre<T>::value;
    const int32_t *__restrict__ fx = g.fx; const float *__restrict__ wx = g.wx;
    const int32_t *__restrict__ fy = g.fy; const float *__restrict__ wy = g.wy;
    const int tx = g.tx, ty = g.ty, nv = g.nv;
    float *wtab = (float *)lsm;                                   // [nrows][T]
    chv_u32x4 *stage = (chv_u32x4 *)(lsm + lanczos_wtab_bytes(rows_per_wave, T));      // [2][nv]
    const int lane = threadIdx.x;
    const int ox0 = strip * 64, j0 = chunk * rows_per_wave;
    if (ox0 >= dst.w || j0 >= dst.h) return;
    const int nrows = min(rows_per_wave, dst.h - j0);
    const int x = ox0 + lane, xe = min(x, dst.w - 1);
    const int col0 = cld<int32_t>((uint64_t)(uintptr_t)(fx + ox0));
    const int col0a = col0 & ~3;                                  // (rounds towards -inf: the staged row starts on a vector of the source row)
    const int cb = gld<int32_t>(fx + xe) - col0a;                 // tap 0 of this lane, in texels from the start of the staged row
    float wr[T];
#pragma unroll
    for (int k = 0; k < T; k++) {
        const float wk = gld<float>(wx + (size_t)xe * tx + min(k, tx - 1));
        wr[k] = k < tx ? wk : 0.f;
    }
    const int row0 = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0));
    // a staged vector that sticks out of the row: the lane loads the row's first / last vector instead and picks CLAMP_TO_EDGE texels from it
    const bool edge = col0a < 0 || col0a + 4 * nv > src.w;        // (uniform)
    const int vc = col0a + 4 * lane, vcc = min(max(vc, 0), src.w - 4);
    const bool loader = lane < nv;
    auto fix = [&](chv_u32x4 L) {
        auto pick = [&](int k) {
            const int i2 = min(max(vc + k, 0), src.w - 1) - vcc;
            return i2 <= 0 ? L.x : i2 == 1 ? L.y : i2 == 2 ? L.z : L.w;
        };
        chv_u32x4 r = { pick(0), pick(1), pick(2), pick(3) };
        return r;
    };
    lanczos_fill_wtab<T>(wtab, wy, ty, j0, nrows, lane);
    // (the load writes its destination registers some time AFTER the statement: the asm names the prefetch slot itself as its output, with
    // no temporary in between that the compiler could copy from before the data has landed; tools/check_inflight.py walks the object)
#define RGB_ISSUE(SLOT, S) do { const int sy_ = min(max(row0 + (S), 0), src.h - 1); \
                                const uint8_t *p_ = src.ptr + (size_t)sy_ * src.pitch + (size_t)vcc * 4; \
                                asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(SLOT) : "v"(p_) : "memory"); } while (0)
    chv_u32x4 pre[PRE];
#pragma unroll
    for (int p = 0; p < PRE; p++) pre[p] = chv_u32x4{ 0u, 0u, 0u, 0u };
    if (loader) {
#pragma unroll
        for (int p = 0; p < PRE; p++) RGB_ISSUE(pre[p], p);
    }
    float4 h[T];
#pragma unroll
    for (int t = 0; t < T; t++) h[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t tap0 = (uint32_t)cb * 4u;
    const int S = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0 + nrows - 1)) - row0 + ty;       // source rows this strip filters
    int jcur = 0, fcur = 0;                                       // next output row to finish, its first source row (fy[j0] - row0 = 0)
    for (int gi = 0; gi * T < S; gi++) {
        auto body = [&](auto tc) -> bool {
            constexpr int t = decltype(tc)::value;
            const int s = gi * T + t;
            if (s >= S) return false;                             // (uniform)
            if (loader) {
                asm volatile("s_waitcnt vmcnt(%1)" : "+v"(pre[t % PRE]) : "n"(PRE - 1) : "memory");
                stage[(t & 1) * nv + lane] = edge ? fix(pre[t % PRE]) : pre[t % PRE];
                RGB_ISSUE(pre[t % PRE], s + PRE);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            // horizontal pass: T texels from the ring (cb + T - 1 < 4 * nv: the ring is sized for T), those beyond tx with weight 0
            const uint32_t *row = (const uint32_t *)((const uint8_t *)(stage + (t & 1) * nv) + tap0);
            uint32_t e[T];
#pragma unroll
            for (int k = 0; k < T; k++) e[k] = row[k];
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < T; k++) {
                acc.x = __builtin_fmaf(wr[k], (float)(e[k] & 255), acc.x);
                acc.y = __builtin_fmaf(wr[k], (float)((e[k] >> 8) & 255), acc.y);
                acc.z = __builtin_fmaf(wr[k], (float)((e[k] >> 16) & 255), acc.z);
                acc.w = __builtin_fmaf(wr[k], (float)(e[k] >> 24), acc.w);
            }
            h[t] = acc;
            // output rows whose last source row this was: source rows s - T + 1 .. s are window rows (t + 1) % T, (t + 2) % T, ...; the
            // filter's ty rows are the window's last ty
            while (jcur < nrows && fcur + ty - 1 == s) {          // (uniform; at most once per source row when reducing)
                const float2 *wrow = (const float2 *)(wtab + jcur * T);
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int k = 0; k < T; k += 2) {
                    const float2 wk = wrow[k >> 1];
                    const float4 h0 = h[(t + 1 + k) % T], h1 = h[(t + 2 + k) % T];
                    o.x = __builtin_fmaf(wk.x, h0.x, o.x);
                    o.y = __builtin_fmaf(wk.x, h0.y, o.y);
                    o.z = __builtin_fmaf(wk.x, h0.z, o.z);
                    o.w = __builtin_fmaf(wk.x, h0.w, o.w);
                    o.x = __builtin_fmaf(wk.y, h1.x, o.x);
                    o.y = __builtin_fmaf(wk.y, h1.y, o.y);
                    o.z = __builtin_fmaf(wk.y, h1.z, o.z);
                    o.w = __builtin_fmaf(wk.y, h1.w, o.w);
                }
                if (x < dst.w) gst<uint32_t>(dst.ptr + (size_t)(j0 + jcur) * dst.pitch + (size_t)x * 4, pack_codes(o.x, o.y, o.z, o.w));
                jcur++;
                if (jcur < nrows) fcur = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0 + jcur)) - row0;
            }
            return true;
        };
        lanczos_all_of(body, std::make_integer_sequence<int, T>{});
    }
#pragma unroll
    for (int p = 0; p < PRE; p++) asm volatile("s_waitcnt vmcnt(0)" : "+v"(pre[p]) :: "memory");      // (nothing leaves in flight)
#undef RGB_ISSUE
}

// ---------------------------------------------------------------------------------------------------------------------
// rgb_tile — any tap counts, any source size.  A block makes g.tw output columns x 4 output rows: the horizontal pass reads its taps from
// global memory (CLAMP_TO_EDGE on the texel index) and leaves one float4 per (source row, column) in LDS, the vertical pass runs out of it.
constexpr int RT_H = 4, RT_W_WIDE = 32, RT_W_NARROW = 8;
typedef uint32_t rgb_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float rgb_f32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

CHV_DEV void rgb_tile(const RgbGeom &g, const DPlane &dst, const DPlane &src, int bx, int by, uint8_t *lsm) {
    float4 *hrow = (float4 *)lsm;                                  // [max_rows][tw]
    const int32_t *__restrict__ fx = g.fx; const float *__restrict__ wx = g.wx;
    const int32_t *__restrict__ fy = g.fy; const float *__restrict__ wy = g.wy;
    const int tx = g.tx, ty = g.ty, tw = g.tw;
    const int ox0 = bx * tw, oy0 = by * RT_H;
    if (ox0 >= dst.w || oy0 >= dst.h) return;
    const int oy_last = min(oy0 + RT_H, dst.h) - 1;
    const int row0 = gld<int32_t>(fy + oy0);
    const int nrows = min(gld<int32_t>(fy + oy_last) + ty - row0, g.max_rows);
    const int tid = threadIdx.x;
    for (int e = tid; e < nrows * tw; e += 256) {
        const int r = e / tw, i = e - r * tw;
        const int xe = min(ox0 + i, dst.w - 1);
        const int f = gld<int32_t>(fx + xe);
        const float *w = wx + (size_t)xe * tx;
        const uint8_t *rowp = src.ptr + (size_t)min(max(row0 + r, 0), src.h - 1) * src.pitch;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        auto tap = [&](float wk, uint32_t t) {
            acc.x = __builtin_fmaf(wk, (float)(t & 255), acc.x);
            acc.y = __builtin_fmaf(wk, (float)((t >> 8) & 255), acc.y);
            acc.z = __builtin_fmaf(wk, (float)((t >> 16) & 255), acc.z);
            acc.w = __builtin_fmaf(wk, (float)(t >> 24), acc.w);
        };
        int k = 0;
        // all taps inside the row: four texels per load (4-byte aligned 16-byte loads), the same taps in the same order
        // (three loads of texels and their weights in flight per trip: taken one by one, a thread's taps are a chain of memory latencies)
        if (f >= 0 && f + tx <= src.w) {
            auto group = [&](auto nc) {
                constexpr int N = decltype(nc)::value;
                rgb_u32x4_a4 t4[N];
                rgb_f32x2_a4 wa[N], wb[N];
#pragma unroll
                for (int u = 0; u < N; u++) {
                    t4[u] = *(const CHV_GLOBAL rgb_u32x4_a4 *)(uintptr_t)(rowp + (size_t)(f + k + 4 * u) * 4);
                    wa[u] = *(const CHV_GLOBAL rgb_f32x2_a4 *)(uintptr_t)(w + k + 4 * u);
                    wb[u] = *(const CHV_GLOBAL rgb_f32x2_a4 *)(uintptr_t)(w + k + 4 * u + 2);
                }
#pragma unroll
                for (int u = 0; u < N; u++) { tap(wa[u].x, t4[u].x); tap(wa[u].y, t4[u].y); tap(wb[u].x, t4[u].z); tap(wb[u].y, t4[u].w); }
                k += 4 * N;
            };
            while (k + 12 <= tx) group(std::integral_constant<int, 3>{});
            while (k + 4 <= tx) group(std::integral_constant<int, 1>{});
        }
        for (; k < tx; k++) tap(gld<float>(w + k), gld<uint32_t>(rowp + (size_t)min(max(f + k, 0), src.w - 1) * 4));
        hrow[e] = acc;
    }
    __syncthreads();
    if (tid < tw * RT_H) {
        const int j = tid / tw, i = tid - j * tw;
        const int x = ox0 + i, oy = oy0 + j;
        if (x < dst.w && oy < dst.h) {
            const int rbase = gld<int32_t>(fy + oy) - row0;
            const float *w = wy + (size_t)oy * ty;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < ty; k++) {
                const float wk = gld<float>(w + k);
                const float4 hk = hrow[(rbase + k) * tw + i];
                o.x = __builtin_fmaf(wk, hk.x, o.x);
                o.y = __builtin_fmaf(wk, hk.y, o.y);
                o.z = __builtin_fmaf(wk, hk.z, o.z);
                o.w = __builtin_fmaf(wk, hk.w, o.w);
            }
            gst<uint32_t>(dst.ptr + (size_t)oy * dst.pitch + (size_t)x * 4, pack_codes(o.x, o.y, o.z, o.w));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The host half: one rung's route and launch numbers, from its geometry alone.

// vectors of one staged source row of a strip whose lanes read `taps` texels each: fx[x + 63] - fx[x] <= floor(63 scale) + 1, 3 texels of
// alignment in front (launch_lanczos's formula)
inline int rgb_row_vectors(int dw, int sw, int taps) {
    const double sx = (double)sw / (double)dw;
    return ((int)(63 * sx) + 1 + 3 + taps + 3) / 4 + 1;
}

// THE routing rule.  Strip route (true) iff no axis has more than 22 taps, the source is at least one vector wide and the staged row of the
// rung's OWN tx fits one vector per lane.  Tile route otherwise.  (A 22-tap rung between 3.603:1 and 3.667:1 has 65 vectors: tile.)
inline bool rgb_strip_route(int dw, int sw, int tx, int ty) {
    return std::max(tx, ty) <= 22 && sw >= 4 && rgb_row_vectors(dw, sw, tx) <= 64;
}

// (a strip rung's own body is lanczos_tap_class of its larger tap count.  The KERNEL of a strip launch is <12> when no strip rung of it has a
// class above 12, else <22>; it is allocated the registers of its largest body.  Rows per wave: lanczos_strip_rows over the sum of the
// launch's rungs, at most RS_MAX_ROWS.)

// tile route: the rows of the LDS array and the tile's width — 32 columns where that many float4 per row fit 64 KB, else 8, which the
// refusal above bounds (max_rows * 8 * 16 <= 160 KB; with at most 256 taps max_rows <= 386, so 8 columns always fit 64 KB)
inline void rgb_tile_dims(int dh, int sh, int ty, int *max_rows, int *tw, size_t *lds) {
    const double sy = (double)sh / (double)dh;
    *max_rows = (int)((RT_H - 1) * sy + 2) + ty;
    *tw = (size_t)*max_rows * RT_W_WIDE * sizeof(float4) <= 64 * 1024 ? RT_W_WIDE : RT_W_NARROW;
    *lds = (size_t)*max_rows * *tw * sizeof(float4);
}

}  // namespace chv
