// lanczos_planar_body.hip.h — the row code of the planar Lanczos-3 resampler, shared by the units that launch it:
// kernels_lanczos_planar.hip.cpp (chv_scale_lanczos on NV12 / y420p pictures: one geometry per launch) and
// kernels_lanczos_planar_ladder.hip.cpp (chv_scale_lanczos_ladder: up to eight geometries per launch).  What differs between the two is how a
// block finds its work; the bytes come from here.
//
// Both bodies see a plane as rows of BYTE columns: output byte b of a row belongs to texel b / C, component b % C, and its taps are the
// source bytes (first[b / C] + k) * C + b % C — a stride of C bytes.  A 2-component plane is therefore the 1-component body with a tap
// stride of two, and one lane owns one output byte whatever the plane is.
//
//   planar_strip<T, C>   every tap count of the launch's geometry <= T <= 22: one WAVE per strip of 64 output bytes x `rows` output rows, in
//                        the manner of lanczos3_strip<T>: source rows staged through a two-row LDS ring with 16-byte loads (issued and
//                        awaited by hand on vector-aligned planes), the horizontal results of the last T source rows in a window of T floats
//                        in the lane's registers, the strip's vertical weights in LDS, a dword store per quad, no block barrier, no scratch.
//   planar_tile          everything else: 32 x 4 output bytes per 256-thread block, horizontal pass from global memory into LDS, vertical
//                        pass out of it.  Simple on purpose.
//
// The host half — which route a geometry takes, its launch numbers, the refusal — is here too, so that no launcher restates it.
#pragma once
#include "pixel_math.hip.h"
#include "lanczos_planar.h"

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>

#pragma clang fp contract(off)

namespace chv {

// what a block needs to know about the plane it works on (kernel arguments: read through the constant address space with the plane's index,
// never by indexing a private copy of the argument)
struct PlanarPlane {
    const int32_t *fx; const float *wx;
    const int32_t *fy; const float *wy;
    DPlane dst, src;                  // picture 0's (a batch reads its own from the descriptor list)
    int32_t tx, ty;
    int32_t strips, chunks;           // blocks along x and y
    int32_t nv;                       // strip kernel: 16-byte vectors of one staged source row
    int32_t max_rows;                 // tile kernel: rows of the LDS array
    int32_t first;                    // blocks of this picture's planes in front of this one
    int32_t pad;
};

template <typename F, int... Is>
CHV_DEV bool planar_all_of(F &&f, std::integer_sequence<int, Is...>) { return (... && f(std::integral_constant<int, Is>{})); }

// bytes a lane's dword reads cover past its first tap's dword: taps at byte offsets o + k * C, o = 0..3, k < T
template <int T, int C> struct PlanarReads { static constexpr int ND = (T * C - C + 7) / 4; };

constexpr int PS_MAX_ROWS = 64;      // output rows per wave at most: their vertical weights live in LDS
constexpr size_t planar_wtab_bytes(int rows, int T) { return ((size_t)rows * T * sizeof(float) + 15) & ~(size_t)15; }
template <int T> struct PlanarPre { static constexpr int value = T % 4 == 0 ? 4 : T % 3 == 0 ? 3 : 2; };      // hand-awaited prefetch depth: a divisor of T
constexpr int PS_PRE = 2;            // source rows in flight (registers) ahead of the row being filtered

// One strip of one plane with C components: 64 output BYTE columns, rows [chunk * rows, ...).  tx, ty <= T: the taps beyond a table's count
// read a staged byte with weight 0 in the horizontal pass (fma(0, finite, acc) == acc), and the vertical pass walks the whole window with
// the weights of the rows older than ty set to 0 (the chain still starts at 0 and stays there until the first real tap) — window indices
// stay static whatever the plane's tap counts are.
template <int T, int C>
CHV_DEV void planar_strip(const PlanarPlane &g, int strip, int chunk, int rows_per_wave, uint8_t *lsm) {
    constexpr int ND = PlanarReads<T, C>::ND, NA = ND - 1;
    const DPlane dst = g.dst, src = g.src;
    const int32_t *__restrict__ fx = g.fx; const float *__restrict__ wx = g.wx;
    const int32_t *__restrict__ fy = g.fy; const float *__restrict__ wy = g.wy;
    const int tx = g.tx, ty = g.ty, nv = g.nv;
    const int lane = threadIdx.x;
    const int wb = dst.w * C, sb = src.w * C;                      // bytes of an output row, of a source row
    const int ox0 = strip * 64, j0 = chunk * rows_per_wave;
    if (ox0 >= wb || j0 >= dst.h) return;
    const int nrows = min(rows_per_wave, dst.h - j0);
    const int xb = ox0 + lane, xe = min(xb, wb - 1);
    const int xt = C == 2 ? xe >> 1 : xe, comp = xe & (C - 1);
    const int b0 = cld<int32_t>((uint64_t)(uintptr_t)(fx + ox0 / C)) * C;
    const int b0a = b0 & ~15;                                      // (rounds towards -inf: the staged row starts on a 16-byte vector of the source row)
    const int cbyte = gld<int32_t>(fx + xt) * C + comp - b0a;                     // tap 0 of this lane, in bytes from the start of the staged row
    float wr[T];
#pragma unroll
    for (int k = 0; k < T; k++) {
        const float wk = gld<float>(wx + (size_t)xt * tx + min(k, tx - 1));
        wr[k] = k < tx ? wk : 0.f;
    }
    const int row0 = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0));
    // 16-byte loads need a 4-byte aligned address: the plane's start and pitch decide (uniform), then every vector that lies inside the row's
    // bytes; all other vectors — those that stick out of the row, every vector of a plane placed at an odd byte — are gathered byte by byte
    // with CLAMP_TO_EDGE on the texel index.  Nothing outside [row start, row start + row bytes) is ever read.
    const bool vec_ok = ((((uintptr_t)src.ptr) | (uint32_t)src.pitch) & 3) == 0;
    const int vb = b0a + 16 * lane;
    const bool loader = lane < nv;
    const bool vec_lane = vec_ok && vb >= 0 && vb + 16 <= sb;
    auto load_row = [&](int s) -> chv_u32x4 {
        const int sy = min(max(row0 + s, 0), src.h - 1);
        const uint8_t *rowp = src.ptr + (size_t)sy * src.pitch;
        if (vec_lane) return *(const CHV_GLOBAL chv_u32x4 *)(uintptr_t)(rowp + vb);
        // (sixteen loads in flight at once: a strip on the picture's edge must not take sixteen latencies per row)
        uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int bi = vb + i;
            const int ci = C == 2 ? 2 * min(max(bi >> 1, 0), src.w - 1) + (bi & 1) : min(max(bi, 0), sb - 1);
            const uint32_t byte = (uint32_t)gld_at<uint8_t>(rowp, (uint32_t)ci) << (8 * (i & 3));
            if (i < 4) d0 |= byte; else if (i < 8) d1 |= byte; else if (i < 12) d2 |= byte; else d3 |= byte;
        }
        return chv_u32x4{ d0, d1, d2, d3 };
    };
    chv_u32x4 *stage = (chv_u32x4 *)(lsm + planar_wtab_bytes(rows_per_wave, T));      // [2][nv]
    const uint32_t tap0 = (uint32_t)cbyte & ~3u, sh = (uint32_t)cbyte & 3u;
    const int pad = T - ty;                                        // window rows in front of a vertical filter's first tap
    const int S = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0 + nrows - 1)) - row0 + ty;       // source rows this strip filters
    // a dword store per quad wherever the target allows it: plane start and pitch 4-byte aligned (uniform), quad inside the row
    const bool st_vec = ((((uintptr_t)dst.ptr) | (uint32_t)dst.pitch) & 3) == 0;
    const bool st_quad = st_vec && (xb | 3) < wb;
    // The vertical weights of the strip's output rows, zero-padded in front to the window's T rows, go to LDS before the row loop (after it every
    // wait for a global load would also wait for the row prefetch: one counter); the vertical chain reads a row of them at one address for all lanes.
    float *wtab = (float *)lsm;                                    // [nrows][T]
    // (eight loads in flight per trip: left rolled, the fill is a chain of as many memory latencies as a lane has entries)
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
    // FAST (uniform per plane): the plane's start and pitch are multiples of 4 and its row bytes a multiple of 16, so every staged vector lies
    // either wholly inside the row's bytes or wholly outside.  A lane outside loads the row's first / last vector instead and replicates its
    // edge texel (CLAMP_TO_EDGE) when it stages it.  The row loads are issued and awaited BY HAND, PRE rows ahead, as in lanczos3_strip<T>: gfx950 counts
    // loads and stores in one counter and completes them out of order with respect to each other, so with the output stores in the loop the
    // compiler drains the counter before every use of a prefetched row and the prefetch hides nothing.  Loads complete in order among
    // themselves: once at most PRE - 1 operations are outstanding, the oldest of PRE loads has arrived whatever the stores did.  The loop holds
    // no other vector load (tables come through the scalar unit and LDS).  tools/check_inflight.py walks the object for touches of a slot
    // in flight (tests/test_lanczos_planar_contract.py).  Every other plane keeps compiler-managed loads and the byte gather.
    const bool fast = vec_ok && sb >= 16 && (sb & 15) == 0;
    const bool edge = b0a < 0 || b0a + 16 * nv > sb;               // (uniform) some staged vector lies outside the row
    const int vbc = min(max(vb, 0), sb - 16);                      // (FAST only) the vector this lane loads
    auto fix = [&](chv_u32x4 v) -> chv_u32x4 {                     // (FAST only) the staged vector of a lane outside the row: its edge texel, 16 / C times
        if (vb == vbc) return v;
        const uint32_t rep = vb < 0 ? (C == 2 ? (v.x & 0xffffu) * 0x00010001u : (v.x & 255u) * 0x01010101u)
                                    : (C == 2 ? (v.w >> 16) * 0x00010001u : (v.w >> 24) * 0x01010101u);
        return chv_u32x4{ rep, rep, rep, rep };
    };
    auto rows = [&](auto fastc) {
    constexpr bool FAST = decltype(fastc)::value;
    constexpr int PRE = FAST ? PlanarPre<T>::value : PS_PRE;
#define PS_ISSUE(SLOT, S) do { const int sy_ = min(max(row0 + (S), 0), src.h - 1); \
                               const uint8_t *p_ = src.ptr + (size_t)sy_ * src.pitch + vbc; \
                               asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(SLOT) : "v"(p_) : "memory"); } while (0)
    chv_u32x4 pre[PRE];
#pragma unroll
    for (int p = 0; p < PRE; p++) pre[p] = chv_u32x4{ 0u, 0u, 0u, 0u };
    if (loader) {
#pragma unroll
        for (int p = 0; p < PRE; p++) { if constexpr (FAST) PS_ISSUE(pre[p], p); else pre[p] = load_row(p); }
    }
    float h[T];
#pragma unroll
    for (int t = 0; t < T; t++) h[t] = 0.f;
    int jcur = 0, fcur = 0;                                        // next output row to finish, its first source row (fy[j0] - row0 = 0)
    for (int gi = 0; gi * T < S; gi++) {
        auto body = [&](auto tc) -> bool {
            constexpr int t = decltype(tc)::value;
            const int s = gi * T + t;
            if (s >= S) return false;                              // (uniform)
            if (loader) {
                if constexpr (FAST) {
                    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(pre[t % PRE]) : "n"(PRE - 1) : "memory");
                    stage[(t & 1) * nv + lane] = edge ? fix(pre[t % PRE]) : pre[t % PRE];
                    PS_ISSUE(pre[t % PRE], s + PRE);
                } else {
                    stage[(t & 1) * nv + lane] = pre[t % PRE];
                    pre[t % PRE] = load_row(s + PRE);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            // horizontal pass of this lane's byte column: aligned dwords from the ring, shifted so that tap 0 is byte 0
            const uint32_t *row = (const uint32_t *)((const uint8_t *)(stage + (t & 1) * nv) + tap0);
            uint32_t raw[ND], al[NA];
#pragma unroll
            for (int i = 0; i < ND; i++) raw[i] = row[i];
#pragma unroll
            for (int i = 0; i < NA; i++) al[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], sh);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < T; k++) {
                const uint32_t word = C == 2 ? al[k >> 1] : al[k >> 2];
                const uint32_t byte = C == 2 ? (word >> (16 * (k & 1))) & 255u : (word >> (8 * (k & 3))) & 255u;
                acc = __builtin_fmaf(wr[k], (float)byte, acc);
            }
            h[t] = acc;
            // output rows whose last source row this was: source rows s - T + 1 .. s are window rows (t + 1) % T, (t + 2) % T, ...
            while (jcur < nrows && fcur + ty - 1 == s) {           // (uniform; at most once per source row when reducing)
                const float2 *wrow = (const float2 *)(wtab + jcur * T);
                float o = 0.f;
#pragma unroll
                for (int k = 0; k < T; k += 2) {
                    const float2 wk = wrow[k >> 1];
                    o = __builtin_fmaf(wk.x, h[(t + 1 + k) % T], o);
                    o = __builtin_fmaf(wk.y, h[(t + 2 + k) % T], o);
                }
                // the lane's code at its byte of the quad's dword, then the quad's four bytes in every lane of it (two quad-permute DPP moves)
                uint32_t w = 0;
                asm("v_cvt_pk_u8_f32 %0, %1, %2, %0" : "+v"(w) : "v"(o), "v"(lane & 3));
                uint8_t *orow = dst.ptr + (size_t)(j0 + jcur) * dst.pitch;
                if (st_vec) {
                    uint32_t q = w | (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0xB1, 0xF, 0xF, false);     // quad_perm [1, 0, 3, 2]
                    q |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)q, 0x4E, 0xF, 0xF, false);                  // quad_perm [2, 3, 0, 1]
                    if (st_quad) { if ((lane & 3) == 0) gst<uint32_t>(orow + xb, q); }
                    else if (xb < wb) gst<uint8_t>(orow + xb, (uint8_t)(w >> (8 * (lane & 3))));                  // the row's last, partial quad
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
    if constexpr (FAST) {                                          // (the rows requested past the strip's last one: nothing leaves in flight)
#pragma unroll
        for (int p = 0; p < PRE; p++) asm volatile("s_waitcnt vmcnt(0)" : "+v"(pre[p]) :: "memory");
    }
#undef PS_ISSUE
    };
    if (fast) rows(std::true_type{}); else rows(std::false_type{});
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

// The 4-component entry's refusal (launch_lanczos: the 8 x 4 tile's staged source beyond 160 KB), evaluated on this plane's own sizes
inline bool planar_refuses(const DPlane &d, const DPlane &s, int tx, int ty) {
    const double sy = (double)s.h / (double)d.h, sx = (double)s.w / (double)d.w;
    const int max_rows = (int)(3 * sy + 2) + ty;
    const int max_cols = ((int)(7 * sx + 2) + tx + 3) & ~3;
    return (size_t)max_rows * 8 * 16 + (size_t)max_rows * max_cols * 4 > 160 * 1024;
}

// THE routing rule.  Strip route (true): no plane has more than 22 taps on an axis and no staged row is longer than 64 vectors; *T is then
// the body's tap class over the geometry's largest tap count, every plane's nv is set and *nvmax is their maximum.  Tile route otherwise.
inline bool planar_strip_route(PlanarPlane *pl, int np, int *T, int *nvmax) {
    int tmax = 0;
    for (int p = 0; p < np; p++) tmax = std::max(tmax, std::max(pl[p].tx, pl[p].ty));
    *T = tmax <= 6 ? 6 : tmax <= 8 ? 8 : tmax <= 12 ? 12 : tmax <= 16 ? 16 : 22;
    *nvmax = 0;
    if (tmax > 22) return false;
    for (int p = 0; p < np; p++) {
        PlanarPlane &g = pl[p];
        const int C = g.dst.comps;
        const double sx = (double)g.src.w / (double)g.dst.w;
        // first[x + n] - first[x] <= floor(n scale) + 1 texels over the strip's 64 / C texel columns; 15 bytes of alignment in front,
        // the dword reads of the last column (its T taps, rounded out to dwords) behind
        const int span = ((int)((64 / C - 1) * sx) + 1) * C + (C - 1);
        const int bytes = 15 + span + 4 * (((*T * C - C + 7) / 4) + 1);
        g.nv = (bytes + 15) / 16 + 1;
        *nvmax = std::max(*nvmax, g.nv);
    }
    return *nvmax <= 64;
}

// strip route: every plane's strips; the (strip, output row) pairs of one picture
inline long planar_strip_work(PlanarPlane *pl, int np) {
    long work = 0;
    for (int p = 0; p < np; p++) {
        pl[p].strips = (pl[p].dst.w * pl[p].dst.comps + 63) / 64;
        work += (long)pl[p].strips * pl[p].dst.h;
    }
    return work;
}

// rows per wave from the launch's (strip, output row) pairs: enough waves for three rounds of four per SIMD when the launch is large; a small
// launch gets short chunks instead — every chunk re-filters ty - 2 warm-up rows, but a wave's serial chain is what a lone resize waits for
inline int planar_strip_rows(long work) {
    const long want = 4L * 1024 * 3;
    const long r = (work + want - 1) / want;
    return (int)std::min<long>(std::max<long>(r, 8), PS_MAX_ROWS);
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
