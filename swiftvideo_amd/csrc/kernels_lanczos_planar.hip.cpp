// kernels_lanczos_planar.hip.cpp — separable Lanczos-3 resampler for the planes of 4:2:0 pictures: 1-component planes (luma, the Cb and Cr
// planes of y420p) and the 2-component CbCr plane of NV12.  Plane-wise: every plane is an image of its own, resampled
// with the tables of its own width and height, every component through the chain of kernels_lanczos.hip.cpp (horizontal then vertical pass,
// one fused multiply-add per tap from 0.0f, taps ascending, float intermediate, convert_uchar_sat_rte).  No colour arithmetic.
//
// ONE launch covers every plane of a picture and every picture of a batch chunk: a block's number decodes to (picture, plane, row chunk,
// strip), and every plane brings its own tables and tap counts.
//
// Both kernels see a plane as rows of BYTE columns: output byte b of a row belongs to texel b / C, component b % C, and its taps are the
// source bytes (first[b / C] + k) * C + b % C — a stride of C bytes.  A 2-component plane is therefore the 1-component kernel with a tap
// stride of two, and one lane owns one output byte whatever the plane is.
//
//   planar_lanczos_strip<T>  every plane's tap counts <= T <= 22: one WAVE per strip of 64 output bytes x `rows` output rows, in the manner of
//                            lanczos3_strip<T>: source rows staged through a two-row LDS ring with 16-byte loads (issued and awaited by hand
//                            on vector-aligned planes), the horizontal results of the last T source rows in a window of T floats in the
//                            lane's registers, the strip's vertical weights in LDS, a dword store per quad, no block barrier, no scratch.
//   planar_lanczos_tile      everything else (more than 22 taps on some axis of some plane): 32 x 4 output bytes per block, horizontal
//                            pass from global memory into LDS, vertical pass out of it.  Simple on purpose.
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
struct PlanarArgs {
    PlanarPlane pl[kLanczosPlanarMaxPlanes];
    const DPlane *batch;
    int32_t n_planes, rows;           // rows: output rows per wave (strip kernel)
    int32_t per_picture, total;       // blocks per picture, blocks in all
};
static_assert(sizeof(PlanarArgs) <= 1024, "kernel arguments: 4 KB in all");

struct PlanarBlock {
    PlanarPlane g;
    int picture, bx, by;
};

// (picture, plane, row chunk, strip) of block `idx`; dst / src of a batch come from the descriptor list
CHV_DEV PlanarBlock planar_decode(int idx) {
    const uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const int n_planes = cld<int32_t>(ka + offsetof(PlanarArgs, n_planes));
    const int per = cld<int32_t>(ka + offsetof(PlanarArgs, per_picture));
    const uint64_t batch = cld<uint64_t>(ka + offsetof(PlanarArgs, batch));
    PlanarBlock r;
    r.picture = idx / per;
    const int rem = idx - r.picture * per;
    const int f1 = cld<int32_t>(ka + offsetof(PlanarArgs, pl) + sizeof(PlanarPlane) + offsetof(PlanarPlane, first));
    const int f2 = cld<int32_t>(ka + offsetof(PlanarArgs, pl) + 2 * sizeof(PlanarPlane) + offsetof(PlanarPlane, first));
    const int plane = (n_planes > 2 && rem >= f2) ? 2 : rem >= f1 ? 1 : 0;
    r.g = cld<PlanarPlane>(ka + offsetof(PlanarArgs, pl) + (uint64_t)plane * sizeof(PlanarPlane));
    const int in_plane = rem - r.g.first;
    r.by = in_plane / r.g.strips;
    r.bx = in_plane - r.by * r.g.strips;
    if (batch) {
        const uint64_t pair = batch + ((uint64_t)r.picture * n_planes + plane) * 2 * sizeof(DPlane);
        r.g.dst = cld<DPlane>(pair); r.g.src = cld<DPlane>(pair + sizeof(DPlane));
    }
    return r;
}

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

template <int T>
__global__ __launch_bounds__(64, (T <= 12 ? 5 : 4)) void planar_lanczos_strip(const PlanarArgs a) {
    // XCD-aware numbering, as in lanczos3_strip2: block b runs on XCD b % 8, and every XCD gets one contiguous range of (picture, plane,
    // row chunk, strip) — neighbouring strips and chunks share their halo columns and rows through that XCD's L2
    const int b = blockIdx.x, per_xcd = (a.total + 7) >> 3;
    const int idx = (b & 7) * per_xcd + (b >> 3);
    if ((b >> 3) >= per_xcd || idx >= a.total) return;
    extern __shared__ __attribute__((aligned(16))) uint8_t planar_lsm[];
    const PlanarBlock blk = planar_decode(idx);
    if (blk.g.dst.comps == 2) planar_strip<T, 2>(blk.g, blk.bx, blk.by, a.rows, planar_lsm);
    else planar_strip<T, 1>(blk.g, blk.bx, blk.by, a.rows, planar_lsm);
}

// ---------------------------------------------------------------------------------------------------------------------
// planar_lanczos_tile — any tap counts.  A block makes 32 output byte columns x 4 output rows: the horizontal pass reads its taps from global
// memory (CLAMP_TO_EDGE on the texel index) and leaves one float per (source row, column) in LDS, the vertical pass runs out of it.
constexpr int PT_W = 32, PT_H = 4;

__global__ __launch_bounds__(256) void planar_lanczos_tile(const PlanarArgs a) {
    const int idx = blockIdx.x;
    if (idx >= a.total) return;
    extern __shared__ __attribute__((aligned(16))) uint8_t planar_lsm[];
    float *hrow = (float *)planar_lsm;                             // [max_rows][PT_W]
    const PlanarBlock blk = planar_decode(idx);
    const DPlane dst = blk.g.dst, src = blk.g.src;
    const int32_t *__restrict__ fx = blk.g.fx; const float *__restrict__ wx = blk.g.wx;
    const int32_t *__restrict__ fy = blk.g.fy; const float *__restrict__ wy = blk.g.wy;
    const int tx = blk.g.tx, ty = blk.g.ty, C = dst.comps;
    const int wb = dst.w * C;
    const int ox0 = blk.bx * PT_W, oy0 = blk.by * PT_H;
    if (ox0 >= wb || oy0 >= dst.h) return;
    const int oy_last = min(oy0 + PT_H, dst.h) - 1;
    const int row0 = gld<int32_t>(fy + oy0);
    const int nrows = min(gld<int32_t>(fy + oy_last) + ty - row0, blk.g.max_rows);
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

// The 4-component entry's refusal (launch_lanczos: the 8 x 4 tile's staged source beyond 160 KB), evaluated on this plane's own sizes
static bool planar_refuses(const DPlane &d, const DPlane &s, int tx, int ty) {
    const double sy = (double)s.h / (double)d.h, sx = (double)s.w / (double)d.w;
    const int max_rows = (int)(3 * sy + 2) + ty;
    const int max_cols = ((int)(7 * sx + 2) + tx + 3) & ~3;
    return (size_t)max_rows * 8 * 16 + (size_t)max_rows * max_cols * 4 > 160 * 1024;
}

static hipError_t launch_lanczos_planar(const LanczosPlanarJob &job, hipStream_t stream) {
    if (job.n_planes < 2 || job.n_planes > kLanczosPlanarMaxPlanes || job.n_pictures < 1) return hipErrorInvalidValue;
    PlanarArgs a{};
    a.batch = job.batch;
    a.n_planes = job.n_planes;
    int tmax = 0, nvmax = 0;
    bool strip_route = true;
    for (int p = 0; p < job.n_planes; p++) {
        const LanczosPlaneTables &t = job.tab[p];
        const DPlane &d = job.dst[p], &s = job.src[p];
        if (d.comps != s.comps || (d.comps != 1 && d.comps != 2)) return hipErrorInvalidValue;
        if (planar_refuses(d, s, t.tx, t.ty)) return hipErrorInvalidValue;        // any plane refused: nothing is launched
        PlanarPlane &g = a.pl[p];
        g.fx = t.fx; g.wx = t.wx; g.fy = t.fy; g.wy = t.wy; g.tx = t.tx; g.ty = t.ty;
        g.dst = d; g.src = s;
        tmax = std::max(tmax, std::max(t.tx, t.ty));
    }
    const int T = tmax <= 6 ? 6 : tmax <= 8 ? 8 : tmax <= 12 ? 12 : tmax <= 16 ? 16 : 22;
    if (tmax > 22) strip_route = false;
    if (strip_route) {
        for (int p = 0; p < job.n_planes; p++) {
            PlanarPlane &g = a.pl[p];
            const int C = g.dst.comps;
            const double sx = (double)g.src.w / (double)g.dst.w;
            // first[x + n] - first[x] <= floor(n scale) + 1 texels over the strip's 64 / C texel columns; 15 bytes of alignment in front,
            // the dword reads of the last column (its T taps, rounded out to dwords) behind
            const int span = ((int)((64 / C - 1) * sx) + 1) * C + (C - 1);
            const int bytes = 15 + span + 4 * (((T * C - C + 7) / 4) + 1);
            g.nv = (bytes + 15) / 16 + 1;
            nvmax = std::max(nvmax, g.nv);
        }
        if (nvmax > 64) strip_route = false;
    }
    (void)hipGetLastError();
    if (strip_route) {
        long work = 0;                                              // (strip, output row) pairs of one picture
        for (int p = 0; p < job.n_planes; p++) {
            PlanarPlane &g = a.pl[p];
            g.strips = (g.dst.w * g.dst.comps + 63) / 64;
            work += (long)g.strips * g.dst.h;
        }
        // rows per wave: enough waves for three rounds of four per SIMD when the launch is large; a small launch gets short chunks instead —
        // every chunk re-filters ty - 2 warm-up rows, but a wave's serial chain is what a lone resize waits for
        const long want = 4L * 1024 * 3;
        const long r = (work * job.n_pictures + want - 1) / want;
        a.rows = (int)std::min<long>(std::max<long>(r, 8), PS_MAX_ROWS);
        int first = 0;
        for (int p = 0; p < job.n_planes; p++) {
            PlanarPlane &g = a.pl[p];
            g.chunks = (g.dst.h + a.rows - 1) / a.rows;
            g.first = first;
            first += g.strips * g.chunks;
        }
        a.per_picture = first;
        const long total = (long)first * job.n_pictures;
        if (total > 0x3fffffff) return hipErrorInvalidValue;
        a.total = (int)total;
        dim3 grid((unsigned)(((a.total + 7) / 8) * 8));
        const size_t lds = planar_wtab_bytes(a.rows, T) + (size_t)2 * nvmax * 16;       // the strip's vertical weights, the two-row staging ring
        switch (T) {
        case 6: hipLaunchKernelGGL(planar_lanczos_strip<6>, grid, dim3(64), lds, stream, a); break;
        case 8: hipLaunchKernelGGL(planar_lanczos_strip<8>, grid, dim3(64), lds, stream, a); break;
        case 12: hipLaunchKernelGGL(planar_lanczos_strip<12>, grid, dim3(64), lds, stream, a); break;
        case 16: hipLaunchKernelGGL(planar_lanczos_strip<16>, grid, dim3(64), lds, stream, a); break;
        default: hipLaunchKernelGGL(planar_lanczos_strip<22>, grid, dim3(64), lds, stream, a); break;
        }
        return hipGetLastError();
    }
    int first = 0, rows_max = 0;
    for (int p = 0; p < job.n_planes; p++) {
        PlanarPlane &g = a.pl[p];
        const double sy = (double)g.src.h / (double)g.dst.h;
        g.strips = (g.dst.w * g.dst.comps + PT_W - 1) / PT_W;
        g.chunks = (g.dst.h + PT_H - 1) / PT_H;
        g.max_rows = (int)((PT_H - 1) * sy + 2) + g.ty;
        rows_max = std::max(rows_max, g.max_rows);
        g.first = first;
        first += g.strips * g.chunks;
    }
    a.per_picture = first;
    const long total = (long)first * job.n_pictures;
    if (total > 0x3fffffff) return hipErrorInvalidValue;
    a.total = (int)total;
    const size_t lds = (size_t)rows_max * PT_W * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;                // (not reached: 256 taps and the refusal above bound it by 50 KB)
    hipLaunchKernelGGL(planar_lanczos_tile, dim3((unsigned)a.total), dim3(256), lds, stream, a);
    return hipGetLastError();
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosPlanarRegistrar { LanczosPlanarRegistrar() { register_lanczos_planar_launcher(launch_lanczos_planar); } } g_lanczos_planar_registrar;

}  // namespace chv
