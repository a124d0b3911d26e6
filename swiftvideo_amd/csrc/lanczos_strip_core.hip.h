// lanczos_strip_core.hip.h — THE wave-per-strip row code of the planar Lanczos-3 resamplers: one body, strip_core,
// for a strip of one logical plane.  planar_strip (lanczos_planar_body.hip.h), x420_strip (lanczos_420_body.hip.h), to420_strip
// (lanczos_to_420_body.hip.h), hbd_strip (lanczos_hbd_body.hip.h) and fy_strip (lanczos_from_yuv_body.hip.h) are wrappers of a few lines: each states how its lanes map to source
// bytes (a column description) and where a finished value goes (a sink).
//
// The body sees the target as rows of BYTE columns: output byte b of a row belongs to texel b / OC, and its taps are SS bytes apart in the
// staged source row, from a byte offset the description gives per lane.  One lane owns one output byte whatever the planes are.  One WAVE makes
// a strip of 64 output bytes x `rows` output rows, in the manner of lanczos3_strip<T>: source rows staged through a two-row LDS ring with
// 16-byte loads (issued and awaited by hand on vector-aligned planes), the horizontal results of the last T source rows in a window of T floats
// in the lane's registers, the strip's vertical weights in LDS, no block barrier, no scratch.
#pragma once
#include "lanczos_strip_parts.hip.h"
#include "lanczos_route.h"

#pragma clang fp contract(off)

namespace chv {

// A column description: the compile-time half of how a lane finds its source bytes.  The run-time half is two integers, off0 and off1: the
// byte of tap 0 inside its source texel (with TWO: inside the ring slot) for the first component of a target texel, or the only one, and for
// the second.
//   SS    source tap stride in bytes: 1, 2 or 4.  It also decides the edge replication (a lane outside the row repeats the row's edge TEXEL of SS
//         bytes) and the tap extraction (SS 1, 2: dwords realigned so that tap 0 is byte 0, taps in 8- or 16-bit fields; SS 4: one dword per tap).
//   OC    target bytes per texel, 1 or 2: output byte xe is texel xe / OC, component xe % OC.
//   TWO   the ring slot holds one staged row of EACH of two source planes (g.src, then src2: same size, own start and pitch).
//   WIDE  what a sample is.  kSampleByte: one byte.  kSampleHigh10, kSampleLow10 (SS 2 or 4, even offsets): the little-endian 16-bit word that
//         starts at the tap's byte — the whole field the byte extraction masks to its low byte — as the 10-bit code word >> 6 or word & 1023
//         (DESIGN.md section 4.4.10).  Staging, edge replication, the byte gather and the dwords a lane reads are the byte samples'.
enum StripSample : int { kSampleByte = 0, kSampleHigh10 = 1, kSampleLow10 = 2 };
template <int SS_, int OC_, bool TWO_ = false, int WIDE_ = kSampleByte> struct StripCols {
    static_assert((SS_ == 1 || SS_ == 2 || SS_ == 4) && (OC_ == 1 || OC_ == 2), "tap stride 1, 2 or 4 bytes, 1 or 2 target components");
    static_assert(WIDE_ == kSampleByte || ((WIDE_ == kSampleHigh10 || WIDE_ == kSampleLow10) && SS_ >= 2), "a 16-bit sample needs a tap stride of 2 or 4");
    static constexpr int SS = SS_, OC = OC_, WIDE = WIDE_;
    static constexpr bool TWO = TWO_;
};
// the sample of a tap from the dword shifted so that the tap's first byte is bit 0
template <int WIDE> CHV_DEV uint32_t strip_sample(uint32_t field) {
    if constexpr (WIDE == kSampleHigh10) return (field & 0xffffu) >> 6;
    else if constexpr (WIDE == kSampleLow10) return field & 1023u;
    else return field & 255u;
}

// The sink of the bodies that store bytes: the lane's code at its byte of the quad's dword, then the quad's four bytes in every lane of it (two
// quad-permute DPP moves) and a dword store per quad wherever the target allows it: plane start and pitch 4-byte aligned (uniform), quad
// inside the row.  wb: bytes of an output row, xb: this lane's byte column, j0: the chunk's first row.
struct ByteQuadSink {
    DPlane dst;
    int wb, xb, j0, lane;
    bool st_vec, st_quad;             // dword stores allowed at all; this lane's quad lies inside the row (asked under st_vec only)
    CHV_DEV ByteQuadSink(const DPlane &d, int wb_, int xb_, int j0_)
        : dst(d), wb(wb_), xb(xb_), j0(j0_), lane(threadIdx.x),
          st_vec(((((uintptr_t)d.ptr) | (uint32_t)d.pitch) & 3) == 0), st_quad((xb_ | 3) < wb_) {}
    CHV_DEV void operator()(int jcur, float o) const {
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
    }
};
// (what strip_core asks for: the sink of a strip, opened once the strip knows where it is)
struct OpenByteQuads {
    CHV_DEV ByteQuadSink operator()(const DPlane &dst, int wb, int xb, int j0) const { return ByteQuadSink(dst, wb, xb, j0); }
};

constexpr int PS_MAX_ROWS = 64;      // output rows per wave at most: their vertical weights live in LDS
constexpr int PS_PRE = 2;            // (gathered rows) source rows in flight (registers) ahead of the row being filtered

// One strip of one logical plane: 64 output BYTE columns, rows [chunk * rows, ...).  open(g.dst, bytes of an output row, the lane's byte
// column, the chunk's first row) gives the strip's sink; every finished value goes to sink(row of the chunk, value) before rounding.  False: the
// block lies outside the plane, nothing was done.  g.dst: the target's size in texels of Cols::OC bytes; g.src: the source's in texels of Cols::SS bytes, its start and
// pitch.  tx, ty <= T: the taps beyond a table's count read a staged byte with weight 0 in the horizontal pass (fma(0, finite, acc) == acc),
// and the vertical pass walks the whole window with the weights of the rows older than ty set to 0 (the chain still starts at 0 and stays
// there until the first real tap) — window indices stay static whatever the plane's tap counts are.
template <int T, typename Cols, typename Open>
CHV_DEV bool strip_core(const PlanarPlane &g, const DPlane &src2, int off0, int off1, int strip, int chunk, int rows_per_wave, uint8_t *lsm, Open &&open) {
    constexpr int SS = Cols::SS, OC = Cols::OC, WIDE = Cols::WIDE;
    constexpr bool TWO = Cols::TWO;
    // dwords a lane reads from its first tap's dword on: taps at byte offsets o + k * SS, o = 0..3, k < T (SS == 4: one per tap)
    constexpr int ND = (T * SS - SS + 7) / 4, NA = ND - 1;
    const DPlane dst = g.dst, src = g.src;
    const int32_t *__restrict__ fx = g.fx; const float *__restrict__ wx = g.wx;
    const int32_t *__restrict__ fy = g.fy; const float *__restrict__ wy = g.wy;
    const int tx = g.tx, ty = g.ty, nv = g.nv;                     // nv: vectors of one staged row of ONE source plane
    const int lane = threadIdx.x;
    const int wb = dst.w * OC, sb = src.w * SS;                    // bytes of an output row, of a source row
    const int ox0 = strip * 64, j0 = chunk * rows_per_wave;
    if (ox0 >= wb || j0 >= dst.h) return false;
    const int nrows = min(rows_per_wave, dst.h - j0);
    const int xb = ox0 + lane, xe = min(xb, wb - 1);
    const int xt = OC == 2 ? xe >> 1 : xe;
    const int off = OC == 2 && (xe & 1) ? off1 : off0;             // this lane's byte within a source texel (or ring slot)
    const int b0 = cld<int32_t>((uint64_t)(uintptr_t)(fx + ox0 / OC)) * SS;
    const int b0a = b0 & ~15;                                      // (rounds towards -inf: the staged row starts on a 16-byte vector of the source row)
    const int ring = TWO ? 2 * nv : nv;                            // vectors of one ring slot
    const int cbyte = gld<int32_t>(fx + xt) * SS + off - b0a;       // tap 0 of this lane, in bytes from the start of the ring slot
    float wr[T];
#pragma unroll
    for (int k = 0; k < T; k++) {
        const float wk = gld<float>(wx + (size_t)xt * tx + min(k, tx - 1));
        wr[k] = k < tx ? wk : 0.f;
    }
    const int row0 = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0));
    // Loader lanes: [0, nv) stage the row of g.src, and with TWO [nv, 2 nv) the row of src2.  2 nv <= 64 for every strip-route geometry: at
    // most 22 taps means a scale of at most 11 / 3, so the strip's 32 texel columns span at most 114 source texels, and with 15 bytes of
    // alignment and the last column's dword reads nv <= 12.  (x420_strip_route checks it all the same.)
    const bool second = TWO && lane >= nv;
    const int li = second ? lane - nv : lane;
    const uint8_t *sptr = second ? src2.ptr : src.ptr;
    const int spitch = second ? src2.pitch : src.pitch;
    // 16-byte loads need a 4-byte aligned address: the plane's start and pitch decide (uniform per plane: a plane at an odd byte is gathered,
    // its sibling need not be), then every vector that lies inside the row's bytes; all other vectors — those that stick out of the row, every
    // vector of a plane placed at an odd byte — are gathered byte by byte with CLAMP_TO_EDGE on the texel index, the byte within the texel
    // kept.  Nothing outside [row start, row start + row bytes) is ever read.
    const bool ok1 = ((((uintptr_t)src.ptr) | (uint32_t)src.pitch) & 3) == 0;
    const bool ok2 = !TWO || ((((uintptr_t)src2.ptr) | (uint32_t)src2.pitch) & 3) == 0;
    const bool vec_ok = second ? ok2 : ok1;
    const int vb = b0a + 16 * li;
    const bool loader = lane < ring;
    const bool vec_lane = vec_ok && vb >= 0 && vb + 16 <= sb;
    auto load_row = [&](int s) -> chv_u32x4 {
        const int sy = min(max(row0 + s, 0), src.h - 1);
        const uint8_t *rowp = sptr + (size_t)sy * spitch;
        if (vec_lane) return *(const CHV_GLOBAL chv_u32x4 *)(uintptr_t)(rowp + vb);
        // (sixteen loads in flight at once: a strip on the picture's edge must not take sixteen latencies per row)
        uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int bi = vb + i;
            const int ci = SS == 4 ? 4 * min(max(bi >> 2, 0), src.w - 1) + (bi & 3)
                         : SS == 2 ? 2 * min(max(bi >> 1, 0), src.w - 1) + (bi & 1) : min(max(bi, 0), sb - 1);
            const uint32_t byte = (uint32_t)gld_at<uint8_t>(rowp, (uint32_t)ci) << (8 * (i & 3));
            if (i < 4) d0 |= byte; else if (i < 8) d1 |= byte; else if (i < 12) d2 |= byte; else d3 |= byte;
        }
        return chv_u32x4{ d0, d1, d2, d3 };
    };
    chv_u32x4 *stage = (chv_u32x4 *)(lsm + lanczos_wtab_bytes(rows_per_wave, T));      // [2][ring]
    const uint32_t tap0 = (uint32_t)cbyte & ~3u, sh = (uint32_t)cbyte & 3u;
    const int S = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0 + nrows - 1)) - row0 + ty;       // source rows this strip filters
    auto &&sink = open(dst, wb, xb, j0);
    float *wtab = (float *)lsm;                                    // [nrows][T]
    lanczos_fill_wtab<T>(wtab, wy, ty, j0, nrows, lane);
    // FAST (uniform per target plane): the source planes' starts and pitches are multiples of 4 and the row bytes a multiple of 16, so every
    // staged vector lies either wholly inside the row's bytes or wholly outside.  A lane outside loads its OWN plane's first / last vector
    // instead and replicates its edge texel (CLAMP_TO_EDGE) when it stages it.  With TWO both planes must qualify — one wait covers the loads
    // of both halves.  The row loads are issued and awaited BY HAND, PRE rows ahead, as in lanczos3_strip<T>: gfx950 counts loads and stores in
    // one counter and completes them out of order with respect to each other, so with the output stores in the loop the compiler drains the
    // counter before every use of a prefetched row and the prefetch hides nothing.  Loads complete in order among themselves: once at most
    // PRE - 1 operations are outstanding, the oldest of PRE loads has arrived whatever the stores did.  The loop holds no other vector load
    // (tables come through the scalar unit and LDS).  tools/check_inflight.py walks every unit's object for touches of a slot in flight
    // (tests/test_lanczos_planar_contract.py and its siblings).  Every other plane keeps compiler-managed loads and the byte gather.
    const bool fast = ok1 && ok2 && sb >= 16 && (sb & 15) == 0;
    const bool edge = b0a < 0 || b0a + 16 * nv > sb;               // (uniform) some staged vector lies outside the row
    const int vbc = min(max(vb, 0), sb - 16);                      // (FAST only) the vector this lane loads
    auto fix = [&](chv_u32x4 v) -> chv_u32x4 {                     // (FAST only) the staged vector of a lane outside the row: its edge texel, 16 / SS times
        if (vb == vbc) return v;                                   // (a packed row's whole dword: its other bytes ride along, no lane of this plane reads them)
        const uint32_t rep = vb < 0 ? (SS == 4 ? v.x : SS == 2 ? (v.x & 0xffffu) * 0x00010001u : (v.x & 255u) * 0x01010101u)
                                    : (SS == 4 ? v.w : SS == 2 ? (v.w >> 16) * 0x00010001u : (v.w >> 24) * 0x01010101u);
        return chv_u32x4{ rep, rep, rep, rep };
    };
    auto rows = [&](auto fastc) {
    constexpr bool FAST = decltype(fastc)::value;
    constexpr int PRE = FAST ? LanczosPre<T>::value : PS_PRE;
    // (the load writes its destination registers some time AFTER the statement: the asm names the prefetch slot itself as its output, with
    // no temporary in between that the compiler could copy from before the data has landed)
#define STRIP_ISSUE(SLOT, S) do { const int sy_ = min(max(row0 + (S), 0), src.h - 1); \
                                  const uint8_t *p_ = sptr + (size_t)sy_ * spitch + vbc; \
                                  asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(SLOT) : "v"(p_) : "memory"); } while (0)
    chv_u32x4 pre[PRE];
#pragma unroll
    for (int p = 0; p < PRE; p++) pre[p] = chv_u32x4{ 0u, 0u, 0u, 0u };
    if (loader) {
#pragma unroll
        for (int p = 0; p < PRE; p++) { if constexpr (FAST) STRIP_ISSUE(pre[p], p); else pre[p] = load_row(p); }
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
                    stage[(t & 1) * ring + lane] = edge ? fix(pre[t % PRE]) : pre[t % PRE];
                    STRIP_ISSUE(pre[t % PRE], s + PRE);
                } else {
                    stage[(t & 1) * ring + lane] = pre[t % PRE];
                    pre[t % PRE] = load_row(s + PRE);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            // horizontal pass of this lane's byte column: aligned dwords from the ring
            const uint32_t *row = (const uint32_t *)((const uint8_t *)(stage + (t & 1) * ring) + tap0);
            uint32_t raw[ND];
#pragma unroll
            for (int i = 0; i < ND; i++) raw[i] = row[i];
            float acc = 0.f;
            if constexpr (SS == 4) {                               // tap k is byte sh of dword k
#pragma unroll
                for (int k = 0; k < T; k++) acc = __builtin_fmaf(wr[k], (float)strip_sample<WIDE>(raw[k] >> (8 * sh)), acc);
            } else {                                               // shifted so that tap 0 is byte 0
                uint32_t al[NA];
#pragma unroll
                for (int i = 0; i < NA; i++) al[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], sh);
#pragma unroll
                for (int k = 0; k < T; k++) {
                    const uint32_t word = SS == 2 ? al[k >> 1] : al[k >> 2];
                    const uint32_t byte = strip_sample<WIDE>(SS == 2 ? word >> (16 * (k & 1)) : word >> (8 * (k & 3)));
                    acc = __builtin_fmaf(wr[k], (float)byte, acc);
                }
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
                sink(jcur, o);                                     // the plane's value of (byte column ox0 + lane, row j0 + jcur)
                jcur++;
                if (jcur < nrows) fcur = cld<int32_t>((uint64_t)(uintptr_t)(fy + j0 + jcur)) - row0;
            }
            return true;
        };
        lanczos_all_of(body, std::make_integer_sequence<int, T>{});
    }
    if constexpr (FAST) {                                          // (the rows requested past the strip's last one: nothing leaves in flight)
#pragma unroll
        for (int p = 0; p < PRE; p++) asm volatile("s_waitcnt vmcnt(0)" : "+v"(pre[p]) :: "memory");
    }
#undef STRIP_ISSUE
    };
    if (fast) rows(std::true_type{}); else rows(std::false_type{});
    return true;
}

}  // namespace chv
