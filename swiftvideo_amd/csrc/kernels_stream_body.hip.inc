// kernels_stream_body.hip.inc — stream_body, the device code of the tick_bgra_stream kernels, and what it is built with: included by
// kernels_stream.hip.cpp (the 32 kernels of every eligible launch), kernels_stream_opq.hip.cpp (the opaque-bottom kernels) and
// kernels_stream_carry.hip.cpp (the chroma-carry kernels) and kernels_stream_dn.hip.cpp (their f32-tap form), each of which instantiates its own __global__ wrappers.  How a launch is cut into waves: stream_plan.h.  The kernel's description is at the top of kernels_stream.hip.cpp.
#pragma once
#include "wave_common.hip.h"
#include "switches.h"
#include "stream_plan.h"

#include <algorithm>
#include <type_traits>
#include <cmath>

#pragma clang fp contract(off)

namespace chv {

#ifndef CHV_ST_ABL
#define CHV_ST_ABL 0        // timing-only (wrong pixels): 1 no ring fills, 2 no canvas stores, 4 no layer arithmetic (rings and stores only)
#endif
#ifndef CHV_STREAM_ABSORB
#define CHV_STREAM_ABSORB 1       // 0: the plain form of the colour matrix for every launch (A/B builds)
#endif
#ifndef CHV_STREAM_PMIX
#define CHV_STREAM_PMIX 1
#endif
#ifndef CHV_STREAM_ROWS_FIXED
#define CHV_STREAM_ROWS_FIXED 0
#endif
#ifndef CHV_STREAM_SMALL_WAVES
#define CHV_STREAM_SMALL_WAVES 4800       // waves a small launch is cut into (launch_bgra_stream)
#endif
#ifndef CHV_STREAM_SMALL_ROWS_MAX
#define CHV_STREAM_SMALL_ROWS_MAX 12
#endif
#ifndef CHV_STREAM_MIN_ROWS
#define CHV_STREAM_MIN_ROWS 4
#endif
#ifndef CHV_STREAM_ROUNDS
#define CHV_STREAM_ROUNDS 12      // chunk height: enough chunks for this many rounds of waves.  With one strip per block and untrimmed requests
                                  // short chunks won (neighbouring strips drift apart over a tall chunk and fetch shared lines twice: 240 rows 1.59 ms
                                  // and 1.75x the algorithmic bytes, 30 rows 1.34 ms); with four strips per block and trimmed requests: 3 / 6 / 12 /
                                  // 18 / 24 / 48 rounds (240 .. 16 rows) = 1.294 / 1.256 / 1.250 / 1.276 / 1.282 / 1.347 ms, traffic 1.00x at 60 rows
                                  // (the six-wave kernel of its day).  The uniform rule only: today's five-wave f32-tap kernel is as flat — 24 / 36 / 52 / 60 / 90 /
                                  // 120 / 240 / 720 rows = 1.072 / 1.055 / 1.047 / 1.043 / 1.041 / 1.047 / 1.068 / 1.129 ms — and batches that fill the chip
                                  // several times over leave the rule for a phased plan (stream_plan.h, profiles/stream_plan_notes.md)
#endif
#ifndef CHV_STREAM_WAVES
#define CHV_STREAM_WAVES 6
#endif
#ifndef CHV_STREAM_LDS_MIN
#define CHV_STREAM_LDS_MIN 0      // timing builds (same pixels): a block asks for at least this much LDS — 32768 holds a CU to five blocks of four
                                  // waves, five waves per SIMD, with the device code untouched (profiles/stream_chroma_carry_notes.md section 1)
#endif

constexpr float kRintBias = 8388608.0f;       // 2^23 (stream_body: the rounding between two layers)
constexpr int ST_PITCH = 128;                 // bytes per ring row (8 vectors)
constexpr int ST_YROWS = 8, ST_CROWS = 4;     // ring rows: luma (batches of 4), chroma (batches of 2)
// LDS layout (NL layers): luma [2 batch slots][NL layers][4 rows][128], then chroma [2 batch slots][NL layers][2 rows][128] — the layers of one
// batch slot lie next to each other so that ONE load instruction fills the rows of two layers (luma: 2 x 4 rows x 8 vectors = 64 lanes) or of
// all four (chroma: 4 x 2 x 8): a vector memory instruction occupies the CU's address unit for 16 cycles whatever it moves
// (tools/ubench_vmem.cpp), and with one instruction per layer and plane that unit was a fifth of the kernel's time.
constexpr int ST_YL = 4 * ST_PITCH, ST_CL = 2 * ST_PITCH;       // bytes of one layer inside a batch slot: 512, 256
// Planar sources (y420p: what FFmpeg's software decoders emit, dec.video.ffmpeg.swift:187-221): the chroma region holds U rows and, behind
// them, V rows — each [2 batch slots][NL layers][2 rows][96] (a strip's chroma texels at up to 1.7 : 1 fit six vectors) — filled by one load
// instruction per plane kind (NL x 2 rows x 6 vectors = 48 lanes at four layers).
constexpr int ST_CLP = 2 * ST_CPP;                              // planar chroma: ST_CPP (tick_route.h) bytes per ring row; bytes of one layer inside a batch slot
template <int NL, bool PL> constexpr int st_layer_bytes() { return ST_PITCH * ST_YROWS + (PL ? 2 * 2 * ST_CLP : ST_PITCH * ST_CROWS); }       // per layer: 1536 / 1792
constexpr int ST_TAB = 32;                    // row entries computed at a time (lane = row)
#ifndef CHV_STREAM_BLOCK
#define CHV_STREAM_BLOCK 4
#endif
constexpr int ST_WAVES = CHV_STREAM_BLOCK;    // waves (neighbouring strips) per block

// integer colour matrix on biased codes -> float codes: yuv_to_bgr_floats (pixel_math.hip.h)

// One load instruction: lane -> (layer li, row rr of the batch, vector vec); `p` is the lane's own 16-byte source address, its LDS
// destination is m0 + lane * 16 (tools/probe_lds_dma.cpp).
// (M0 is a reserved register to hipcc: it cannot be named as a clobber — "may lead to undefined behaviour" — so the statement sets it itself
// every time, and tests/test_device_code_contract.py checks on the built code that nothing else in this kernel reads or writes M0.)
CHV_DEV void st_dma(const uint8_t *p, bool active, uint32_t m0) {
    if (active && !(CHV_ST_ABL & 1))
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"(m0), "v"(p) : "memory");
}

// A row's store: the row's address stays on the scalar unit (gst_at asks for the same, and here hipcc adds the lane's offset to it with a
// 64-bit vector add per row instead).  The stores share the counter the ring's loads are awaited by; they only ever make a wait longer.
CHV_DEV void st_store(uint8_t *row, uint32_t off, uint32_t v) {
    asm volatile("global_store_dword %0, %1, %2" :: "v"(off), "v"(v), "s"(row) : "memory");
}

// A layer's twelve tap bytes, read as ONE group and awaited ONCE: left to hipcc every tap is a byte read followed four instructions later
// by an `s_waitcnt lgkmcnt(n)` of its own (45 waits per row at four layers, a wave asleep for an LDS round trip a dozen times per row).
// The reads are issued by hand — hipcc neither counts them nor knows that their destinations are still being written — so the wait
// statement names every destination as "+v": no consumer can be scheduled above it, and tests/test_stream_row_control_contract.py checks on
// the built code that nothing touches a destination between its read and the wait that covers it.  LDS operations of a wave complete in
// order and nothing but LDS reads counts in lgkmcnt inside the row loop (the refill's scalar loads are awaited there): `lgkmcnt(12)` with the
// NEXT layer's group issued behind this one's means "this layer's twelve have arrived".
struct StTaps { uint32_t y00, y10, y01, y11, u00, u10, u01, u11, v00, v10, v01, v11; };
template <int LO, int LC, int LV>
CHV_DEV void st_taps_read(StTaps &t, uint32_t aY00, uint32_t aY10, uint32_t aY01, uint32_t aY11, uint32_t aC00, uint32_t aC10, uint32_t aC01, uint32_t aC11) {
    asm volatile("ds_read_u8 %0, %12 offset:%20\n\tds_read_u8 %1, %13 offset:%20\n\tds_read_u8 %2, %14 offset:%20\n\tds_read_u8 %3, %15 offset:%20\n\t"
                 "ds_read_u8 %4, %16 offset:%21\n\tds_read_u8 %5, %17 offset:%21\n\tds_read_u8 %6, %18 offset:%21\n\tds_read_u8 %7, %19 offset:%21\n\t"
                 "ds_read_u8 %8, %16 offset:%22\n\tds_read_u8 %9, %17 offset:%22\n\tds_read_u8 %10, %18 offset:%22\n\tds_read_u8 %11, %19 offset:%22"
                 : "=&v"(t.y00), "=&v"(t.y10), "=&v"(t.y01), "=&v"(t.y11), "=&v"(t.u00), "=&v"(t.u10), "=&v"(t.u01), "=&v"(t.u11),
                   "=&v"(t.v00), "=&v"(t.v10), "=&v"(t.v01), "=&v"(t.v11)
                 : "v"(aY00), "v"(aY10), "v"(aY01), "v"(aY11), "v"(aC00), "v"(aC10), "v"(aC01), "v"(aC11), "n"(LO), "n"(LC), "n"(LV));
}
// wait until at most YOUNGER LDS reads issued after the group are outstanding: the group has arrived
template <int YOUNGER>
CHV_DEV void st_taps_wait(StTaps &t) {
    asm volatile("s_waitcnt lgkmcnt(%12)"
                 : "+v"(t.y00), "+v"(t.y10), "+v"(t.y01), "+v"(t.y11), "+v"(t.u00), "+v"(t.u10), "+v"(t.u01), "+v"(t.u11), "+v"(t.v00), "+v"(t.v10), "+v"(t.v01), "+v"(t.v11)
                 : "n"(YOUNGER));
}

// The chroma-carry form (CRY, kernels_stream_carry.hip.cpp): 4:2:0 chroma is half height, so at the headline's 1.5 : 1 reduction the chroma
// tap row stays where it was on one canvas row in four and advances by exactly one on the others — the old lower tap row is the new upper
// one.  The lane KEEPS the chroma bytes of the two ring rows it taps, in two sets indexed by the ring row's parity, and reads only the set
// whose row is new to it: 4 bytes per layer on three rows in four, none on the fourth, where the transient form reads 8 on every row.
// A set: [layer][u at tap column 0, u at column 1, v at column 0, v at column 1] of one chroma ring row (NV12: a (u, v) pair per texel).
template <int NL> struct StCarry { uint32_t c[NL][4]; };
static_assert(ST_CL == 256, "the offsets of st_carry_read");
#define CHV_ST_CARRY_LAYER(L, OU, OV) "ds_read_u8 %[c" #L "0], %[a0] offset:" #OU "\n\tds_read_u8 %[c" #L "1], %[a1] offset:" #OU "\n\t" \
                                      "ds_read_u8 %[c" #L "2], %[a0] offset:" #OV "\n\tds_read_u8 %[c" #L "3], %[a1] offset:" #OV "\n\t"
#define CHV_ST_CARRY_REGS(S, L, C) [c##L##0] C((S).c[L][0]), [c##L##1] C((S).c[L][1]), [c##L##2] C((S).c[L][2]), [c##L##3] C((S).c[L][3])
// one ring row's bytes of every layer as ONE group, issued by hand like st_taps_read (a0 / a1: layer 0's U byte at the lane's two tap columns)
template <int NL>
CHV_DEV void st_carry_read(StCarry<NL> &s, uint32_t a0, uint32_t a1) {
    static_assert(NL >= 2 && NL <= 4, "the carry form: two to four layers");
    if constexpr (NL == 2)
        asm volatile(CHV_ST_CARRY_LAYER(0, 0, 1) CHV_ST_CARRY_LAYER(1, 256, 257)
                     : CHV_ST_CARRY_REGS(s, 0, "+v"), CHV_ST_CARRY_REGS(s, 1, "+v") : [a0] "v"(a0), [a1] "v"(a1));
    else if constexpr (NL == 3)
        asm volatile(CHV_ST_CARRY_LAYER(0, 0, 1) CHV_ST_CARRY_LAYER(1, 256, 257) CHV_ST_CARRY_LAYER(2, 512, 513)
                     : CHV_ST_CARRY_REGS(s, 0, "+v"), CHV_ST_CARRY_REGS(s, 1, "+v"), CHV_ST_CARRY_REGS(s, 2, "+v") : [a0] "v"(a0), [a1] "v"(a1));
    else
        asm volatile(CHV_ST_CARRY_LAYER(0, 0, 1) CHV_ST_CARRY_LAYER(1, 256, 257) CHV_ST_CARRY_LAYER(2, 512, 513) CHV_ST_CARRY_LAYER(3, 768, 769)
                     : CHV_ST_CARRY_REGS(s, 0, "+v"), CHV_ST_CARRY_REGS(s, 1, "+v"), CHV_ST_CARRY_REGS(s, 2, "+v"), CHV_ST_CARRY_REGS(s, 3, "+v")
                     : [a0] "v"(a0), [a1] "v"(a1));
}
// a set's registers named as read and written (no instructions): what st_carry_wait ties behind its wait
template <int NL>
CHV_DEV void st_carry_tie(StCarry<NL> &s) {
    if constexpr (NL == 2) asm volatile("" : CHV_ST_CARRY_REGS(s, 0, "+v"), CHV_ST_CARRY_REGS(s, 1, "+v"));
    else if constexpr (NL == 3) asm volatile("" : CHV_ST_CARRY_REGS(s, 0, "+v"), CHV_ST_CARRY_REGS(s, 1, "+v"), CHV_ST_CARRY_REGS(s, 2, "+v"));
    else asm volatile("" : CHV_ST_CARRY_REGS(s, 0, "+v"), CHV_ST_CARRY_REGS(s, 1, "+v"), CHV_ST_CARRY_REGS(s, 2, "+v"), CHV_ST_CARRY_REGS(s, 3, "+v"));
}
// a layer's four luma taps: transient, read on every row (luma advances by one or two rows per canvas row at 1.5 : 1)
struct StLuma { uint32_t y00, y10, y01, y11; };
template <int LO>
CHV_DEV void st_luma_read(StLuma &t, uint32_t aY00, uint32_t aY10, uint32_t aY01, uint32_t aY11) {
    asm volatile("ds_read_u8 %0, %4 offset:%8\n\tds_read_u8 %1, %5 offset:%8\n\tds_read_u8 %2, %6 offset:%8\n\tds_read_u8 %3, %7 offset:%8"
                 : "=&v"(t.y00), "=&v"(t.y10), "=&v"(t.y01), "=&v"(t.y11) : "v"(aY00), "v"(aY10), "v"(aY01), "v"(aY11), "n"(LO));
}
template <int YOUNGER>
CHV_DEV void st_luma_wait(StLuma &t) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(t.y00), "+v"(t.y10), "+v"(t.y01), "+v"(t.y11) : "n"(YOUNGER));
}
// Layer 0's wait: the row's chroma groups (if any) were issued in FRONT of layer 0's luma taps and LDS reads complete in order, so this
// wait covers them as well — both sets are tied behind it, whether this row read them or not.
template <int NL, int YOUNGER>
CHV_DEV void st_carry_wait(StLuma &t, StCarry<NL> &even, StCarry<NL> &odd) {
    st_luma_wait<YOUNGER>(t);
    st_carry_tie<NL>(even);
    st_carry_tie<NL>(odd);
}

// ONE: a launch of one tick whose descriptors are kernel ARGUMENTS (tick_bgra_stream_one below) — `ticks` / `layers` point into the kernarg
// segment, every field is a scalar load at a constant offset from one base, issued together: no tick -> first_layer -> layer chain of
// dependent loads in front of a lone tick's waves, and no descriptor copy in front of the launch.
// ABS: every layer's colour matrix has absorbing biases (csc_fold_absorbed, pixel_math.hip.h; launch_bgra_stream decides)
// OPQ: the bottom layer's opacity is exactly 1 in every tick (kernels_stream_opq.hip.cpp; launch_bgra_stream decides; NL >= 2, ABS only): on the
// cleared canvas its blend RN(code x 1) is the code it already holds as a clamped 16.16 sum, so the layer computes no blend, and layer 1
// takes that sum times its 1 - opacity through one v_fma_mix_f32 per channel (see `ial24`).
// CRY: the chroma taps are carried down the lane from row to row (StCarry above; kernels_stream_carry.hip.cpp: OPQ batch kernels of NV12 sources)
// DN: the taps of the carry form enter full-rate v_fma_f32 / v_fmac_f32 as binary32 denormals instead of v_fma_mix_f32 as binary16 ones
// (cs_mix_d, pixel_math.hip.h; kernels_stream_dn.hip.cpp): the column weights carry 2^127 where they carry kTapScale, the samples leave the
// taps scaled by 2^-22 and the 2^22 rides on the add that converts them (yuv_to_bgr_fixed_absorbed_d).  Same bytes; the blend is untouched.
// CUT, how the launch is cut into waves: a batch's StreamPlan (stream_plan.h: up to four phases of falling chunk heights, a kernel argument read
// by scalar loads; only tick, y0, nrows and strip live past the prologue), the by-value lone tick's StreamUniform (one grid, its old arguments)
struct StreamUniform { int chunks_y, rows; };
template <int NL, bool ONE, bool PL, bool ABS, bool OPQ = false, bool CRY = false, bool DN = false, class CUT>
CHV_DEV void stream_body(const DTick *__restrict__ ticks, const DLayer *__restrict__ layers, int strips_x, const CUT &cut) {
    // ST_WAVES independent waves per block, on neighbouring strips (no barrier anywhere): their source windows overlap by a vector or two,
    // and waves of one block start together on one CU — the shared lines are fetched once (HBM traffic 1.47x -> see profiles/r03_notes.md)
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_all[];
    constexpr int LBYTES = st_layer_bytes<NL, PL>();
    constexpr int CPITCH = PL ? ST_CPP : ST_PITCH, CLB = PL ? ST_CLP : ST_CL;             // chroma ring row, one layer inside a chroma batch slot
    constexpr int VOFF = PL ? 2 * NL * ST_CLP : 1;                                       // from a U sample to its V sample
    constexpr int WBYTES = NL * LBYTES + ST_TAB * (int)(sizeof(uint4) + sizeof(uint32_t));       // (NV12, four layers: 6784 — six blocks of four waves per CU)
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    uint8_t *lds = lds_all + wave * WBYTES;
    uint4 *rowtab = (uint4 *)(lds + NL * LBYTES);                 // [ST_TAB] what vector instructions use: {luma row weight, chroma row weight, 1 - luma, 1 - chroma}
    uint32_t *rowpos = (uint32_t *)(rowtab + ST_TAB);             // [ST_TAB] what the scalar unit uses: luma tap row (16 bits) | chroma tap row (15 bits) << 16 | row inside the picture << 31
    const uint32_t lds0 = (uint32_t)(size_t)lds;                  // LDS byte address of the rings (the DMA's M0)
    static_assert(!OPQ || (NL >= 2 && ABS && CHV_STREAM_PMIX), "the opaque-bottom form: two layers or more, absorbed matrices, binary16 blend inputs");
    static_assert(!CRY || (OPQ && !PL && !ONE && !(CHV_ST_ABL & 4)), "the chroma-carry form: opaque-bottom batch kernels of NV12 sources");
    static_assert(!DN || CRY, "the f32-tap form: the chroma-carry kernels");
    const int lane = threadIdx.x & 63;
    // XCD-aware numbering inside a phase: block b runs on XCD b % 8; an XCD owns a contiguous range of (tick, chunk, group of ST_WAVES strips)
    int tick, y0, rows_per_chunk, strip;
    if constexpr (ONE) {
        static_assert(std::is_same<CUT, StreamUniform>::value, "the by-value lone tick: one uniform grid");
        rows_per_chunk = cut.rows;
        if (!stream_phase_decode(0, 1, cut.chunks_y, cut.rows, strips_x, ST_WAVES, (int)blockIdx.x, wave, tick, y0, strip)) return;
    } else {
        static_assert(std::is_same<CUT, StreamPlan>::value, "a batch: its plan");
        if (!stream_plan_decode(cut, strips_x, ST_WAVES, (int)blockIdx.x, wave, tick, y0, rows_per_chunk, strip)) return;
    }
    const DTick &T = ticks[ONE ? 0 : tick];
    const DLayer *L = layers + (ONE ? 0 : T.first_layer);
    const int x0 = strip * 64;
    if (x0 >= T.W || y0 >= T.H) return;
    const int nrows = min(rows_per_chunk, T.H - y0);
    const DPlane D = T.dst.pl[0];
    const float sx = (float)T.W, sy = (float)T.H;
    const float *U = L[0].u;                                       // (layers 1.. : LF_SAME_GEOM — the same 48 geometry inputs, plane shapes, bounding box)
    const DPlane SY = L[0].src.pl[0], SC = L[0].src.pl[1];

    // ---- this lane's column: tap positions and weights (WaveStrip::setup, wave_common.hip.h) ---------------------------------
    const int x = x0 + lane, xe = min(x, T.W - 1);
    const float nx = ((float)xe / sx) * 2.f - 1.f;
    const float t3 = U[U_TRANSFORM + 15];
    const float t0 = nx * U[U_TRANSFORM + 0] + U[U_TRANSFORM + 3];
    const float b0 = nx * U[U_BORDER + 0] + U[U_BORDER + 3];
    const float u = t0 * U[U_TEXTURE + 0] + t3 * U[U_TEXTURE + 3];
    const int cfl = ((b0 >= 0.f && b0 <= 1.f) ? AX_BORDER : 0) | ((t0 >= 0.f && t0 <= 1.f) ? AX_TX : 0) | ((u >= 0.f && u <= 1.f) ? AX_UV : 0);
    int cy, cc;
    float cya, cca;
    lin_axis_raw(u, SY.w, cy, cya); lin_axis_raw(u, SC.w, cc, cca);
    // first source column of the strip (no flips: lane 0 has the smallest positions), as the start of the staged 128 bytes
    const int cy_first = __builtin_amdgcn_readfirstlane(cy), cc_first = __builtin_amdgcn_readfirstlane(cc);
    const int ycol0 = min(max(cy_first, 0), SY.w - 1) & ~15;
    constexpr int BPC = PL ? 1 : 2;                                                     // bytes per chroma texel of the ring: a U (V) byte / a (U, V) pair
    const int ccol0 = (min(max(cc_first, 0), SC.w - 1) * BPC) & ~15;
    // byte offsets of the two tap columns inside a ring row, CLAMP_TO_EDGE in x; lanes past the staged bytes (columns outside the canvas
    // or outside the picture, never stored / never taken) read whatever is there
    const int oy0 = min(max(min(max(cy, 0), SY.w - 1) - ycol0, 0), ST_PITCH - 1), oy1 = min(max(min(max(cy + 1, 0), SY.w - 1) - ycol0, 0), ST_PITCH - 1);
    const int oc0 = min(max(min(max(cc, 0), SC.w - 1) * BPC - ccol0, 0), CPITCH - BPC), oc1 = min(max(min(max(cc + 1, 0), SC.w - 1) * BPC - ccol0, 0), CPITCH - BPC);
    // (the chroma offsets are even, and a compiler that knows it fuses a pair's U and V byte reads into one 16-bit read and splits it
    // again with two more vector instructions per tap pair: every tap its own byte read is the cheaper form here, r03_notes.md section 2)
    int oc0v = oc0, oc1v = oc1;
    asm("" : "+v"(oc0v), "+v"(oc1v));
    // (DN: kTapScaleD, the largest power of two — see cs_mix_d for the overflow and underflow bounds)
    constexpr float kColScale = DN ? kTapScaleD : kTapScale;
    const float iya = (1.0f - cya) * kColScale, ya = cya * kColScale, ica = (1.0f - cca) * kColScale, ca = cca * kColScale;
    const bool lane_pic = cfl == AX_ALL && x < T.W;
    // 16-byte vectors of a ring row that some tap of the strip can read (the last lane has the largest offsets): the rest is not requested
    const int nvecY = (__builtin_amdgcn_readlane(oy1, 63) >> 4) + 1, nvecC = ((__builtin_amdgcn_readlane(oc1, 63) + BPC - 1) >> 4) + 1;

    // per-layer constants (wave-uniform), read once: the asm statements below clobber "memory", and every descriptor read after one of
    // them would be a fresh scalar load with its latency in the middle of the ring logic
    std::conditional_t<ABS, CscAbsorbed, CscFolded> csc[NL];
    float al[NL], ial[NL], nrb[NL], al24[NL];
    float ial24 = 0.f;
    const uint8_t *planeY[NL], *planeC[NL], *planeV[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) {
        if constexpr (ABS) csc[l] = csc_fold_absorbed(L[l].csc);
        else csc[l] = csc_fold_biased(kCsc[L[l].csc & 3]);
        al[l] = 1.0f * L[l].u[U_OPACITY]; ial[l] = 1.f - al[l];
        // Between two layers the canvas pixel is rounded to codes (what the first layer's store would have kept) and multiplied by the next
        // layer's 1 - opacity.  The rounding is one add of 2^23 (x + 2^23 = 2^23 + rint(x) exactly, ties to even, for 0 <= x < 2^22); taking the
        // 2^23 out again and the multiply are ONE fused multiply-add: fma(x + 2^23, ia, -2^23 ia) rounds the exact (rint(x) + 2^23) ia - 2^23 ia
        // = rint(x) ia — the product the separate multiply rounds — because 2^23 ia is exact (a power of two times a float).  The constant
        // lives in a vector register: a VOP3 instruction reads one scalar operand, and that is the layer's 1 - opacity.
        al24[l] = al[l] * kTapScale;                     // (exact: a power of two; the layer's pixel arrives scaled by 2^-24, see the blend)
        nrb[l] = -kRintBias * ial[l];
        if (!(OPQ && l <= 1)) asm volatile("" : "+v"(nrb[l]));       // (OPQ: layer 1 has no rounding constant to take out, see ial24)
        // OPQ, layer 1: the bottom layer's code arrives as a binary16 (code x 2^-24, exact) and (1 - opacity) x 2^24 is exact, so
        // fma_mix(ial24, code_h, +0) rounds the real number code x (1 - opacity) once — what fma(code + 2^23, ia, -2^23 ia) rounds above
        if (OPQ && l == 1) ial24 = ial[1] * kTapScale;
        planeY[l] = L[l].src.pl[0].ptr; planeC[l] = L[l].src.pl[1].ptr; planeV[l] = L[l].src.pl[PL ? 2 : 1].ptr;
    }
    // this lane's place in a batch: (row, vector) and its byte column, luma and chroma
    // (planar chroma: a layer's two rows of six vectors are twelve lanes)
    const int liC = PL ? (lane * 43) >> 9 : lane >> 4, inC = PL ? lane - liC * 12 : lane & 15;      // lane -> layer, place inside the layer's rows
    static_assert(((63 * 43) >> 9) == 5 && ((47 * 43) >> 9) == 3 && ((48 * 43) >> 9) == 4 && ((11 * 43) >> 9) == 0 && ((12 * 43) >> 9) == 1, "lane / 12");
    const int rrY = (lane >> 3) & 3, rrC = PL ? (inC >= 6 ? 1 : 0) : (lane >> 3) & 1, vecC = PL ? inC - 6 * rrC : lane & 7;
    const int colY = min(ycol0 + 16 * (lane & 7), SY.w - 16), colC = min(ccol0 + 16 * vecC, SC.w * BPC - 16);

    // the chunk's last tap rows: nothing past them is requested (a chunk's overshoot is another wave's first rows: fetched twice)
    int lastY, lastC;
    {
        const int ye = min(y0 + nrows - 1, T.H - 1);
        const float ny = ((float)ye / sy) * 2.f - 1.f;
        const float t1 = ny * U[U_TRANSFORM + 5] + U[U_TRANSFORM + 7];
        const float v = t1 * U[U_TEXTURE + 5] + t3 * U[U_TEXTURE + 7];
        int ry, rc;
        float a_;
        lin_axis_raw(v, SY.h, ry, a_); lin_axis_raw(v, SC.h, rc, a_);
        lastY = __builtin_amdgcn_readfirstlane(ry) + 1; lastC = __builtin_amdgcn_readfirstlane(rc) + 1;
    }
    uint32_t pending = 0u;                                        // the previous row's pixel, stored after this row's wait
    uint32_t alpha_word = 0xFF000000u;                            // img_clear_bgra's pixel; the word the colour bytes are packed into
    asm volatile("" : "+v"(alpha_word));
    // DN: 2^22, what takes the taps' 2^-22 out again, in a vector register of its own like alpha_word and nrb: the fused multiply-add that
    // converts a sample reads its one scalar operand for the layer's bias
    [[maybe_unused]] float unscale = kTapUnscaleD;
    if constexpr (DN) asm volatile("" : "+v"(unscale));
    int issued = 0, seqY = 0, seqC = 0;                           // load instructions issued so far; the count right after the newest luma / chroma batch
    int nextY = 0, nextC = 0, landY = 0, landC = 0, baseY = 0, baseC = 0;      // ring state: rows below next* are requested, below land* have arrived
    // CRY: the carried chroma bytes — ring rows (row - baseC) & 1 == 0 in `cset[0]`, the others in `cset[1]` — and the source row each holds
    // (wave-uniform; no row yet: the chunk's first row reads both)
    [[maybe_unused]] StCarry<CRY ? NL : 2> cset[2] = {};
    [[maybe_unused]] int held0 = 0x40000000, held1 = 0x40000000;
    for (int j = 0; j < nrows; j++) {
        // ---- row entries, ST_TAB at a time: lane = row (WaveStrip::setup) ------------------------------------------------
        if ((j & (ST_TAB - 1)) == 0) {
            wave_lds_fence();
            const int ye = min(y0 + j + min(lane, ST_TAB - 1), T.H - 1);
            const float ny = ((float)ye / sy) * 2.f - 1.f;
            const float t1 = ny * U[U_TRANSFORM + 5] + U[U_TRANSFORM + 7];
            const float b1 = ny * U[U_BORDER + 5] + U[U_BORDER + 7];
            const float v = t1 * U[U_TEXTURE + 5] + t3 * U[U_TEXTURE + 7];
            const int rfl = ((b1 >= 0.f && b1 <= 1.f) ? AX_BORDER : 0) | ((t1 >= 0.f && t1 <= 1.f) ? AX_TX : 0) | ((v >= 0.f && v <= 1.f) ? AX_UV : 0);
            int ry, rc;
            float rya, rca;
            lin_axis_raw(v, SY.h, ry, rya); lin_axis_raw(v, SC.h, rc, rca);
            if (lane < ST_TAB) {
                rowtab[lane] = make_uint4(__float_as_uint(rya), __float_as_uint(rca), __float_as_uint(1.0f - rya), __float_as_uint(1.0f - rca));
                // (rows of the picture: -1 .. plane rows - 1, which the host holds to 16 / 15 signed bits; rows outside it are not stored, and
                // clamped — still rising with the canvas row — they steer the rings as their unclamped values would)
                rowpos[lane] = ((uint32_t)min(max(ry, -32768), 32767) & 0xFFFFu) | (((uint32_t)min(max(rc, -16384), 16383) & 0x7FFFu) << 16) | (rfl == AX_ALL ? 0x80000000u : 0u);
            }
            wave_lds_fence();
        }
        const uint4 re = rowtab[j & (ST_TAB - 1)];
        const int rp = __builtin_amdgcn_readfirstlane((int)rowpos[j & (ST_TAB - 1)]);
        const int ry = (int)((uint32_t)rp << 16) >> 16, rc = (int)((uint32_t)rp << 1) >> 17;
        const bool row_pic = rp < 0;
        // (the row weights and their complements are used by vector instructions only: they stay the broadcast registers the LDS read
        // returned — no v_readfirstlane, and the two subtractions were done once per row by the table's lane)
        const float yb = __uint_as_float(re.x), cbw = __uint_as_float(re.y);
        // ---- residency: source rows ry, ry + 1 (luma) and rc, rc + 1 (chroma) of every layer ------------------------------
        // A ring holds two batches.  The next batch is REQUESTED as soon as the taps have left the older of the two (ry has entered the
        // newer one) and AWAITED only when a tap row reaches it — about two canvas rows later at a 1.5 : 1 reduction, time the other waves
        // of the SIMD fill; waiting right after the request put every wave to sleep for a memory latency every 1.3 rows (pipeline 1.57 ms).
        if (j == 0) {
            baseY = ry; baseC = rc; nextY = ry; nextC = rc; landY = ry; landC = rc;       // the rings start at the chunk's first tap rows
        }
        {
            // Requests are awaited by COUNT: loads complete in order among themselves, so once at most n vector-memory operations are
            // outstanding, where n is the number of loads issued after the batch a tap row needs, that batch has landed — whatever the
            // canvas stores in between did (they share the counter and complete out of order; they can only make the wait longer).
            // A full drain instead would also wait for the other plane's request of a row ago.
            auto await = [&](int younger) {                        // (uniform)
                if (younger <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else if (younger == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
                else if (younger == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                wave_lds_fence();
            };
            const bool needY = ry + 1 >= landY, needC = rc + 1 >= landC;
            const bool wantY = ry + ST_YROWS / 2 >= nextY && nextY <= lastY, wantC = rc + ST_CROWS / 2 >= nextC && nextC <= lastC;     // (uniform)
            // (one test for the rows on which nothing happens — two in five at a 1.5 : 1 reduction: a row's nine uniform branches were a
            // tenth of its time)
            if (needY | needC | wantY | wantC) {
            if (needY) { await(issued - seqY); landY = nextY; }
            if (needC) { await(issued - seqC); landC = nextC; }
            if (wantY || wantC) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // (the taps of the rows being overwritten have been read)
            // (a while: the first row fills both batches; strong vertical reductions skip rows)
            while (ry + ST_YROWS / 2 >= nextY && nextY <= lastY) {
                // four luma rows of every layer, two layers per instruction; the planes of all layers have one shape (LF_SAME_GEOM)
                const uint32_t slot = (uint32_t)((((nextY - baseY) >> 2) & 1) * (NL * ST_YL));
                const int r = min(max(nextY + rrY, 0), SY.h - 1);
                const size_t roff = (size_t)r * SY.pitch + (size_t)colY;
#pragma unroll
                for (int l0 = 0; l0 < NL; l0 += 2) {
                    const uint8_t *pa = planeY[l0], *pb = planeY[l0 + 1 < NL ? l0 + 1 : l0];
                    st_dma((lane < 32 ? pa : pb) + roff, (lane < 32 || l0 + 1 < NL) && (lane & 7) < nvecY && nextY + rrY <= lastY, lds0 + slot + (uint32_t)(l0 * ST_YL));
                }
                nextY += 4; issued += (NL + 1) / 2; seqY = issued;
            }
            while (rc + ST_CROWS / 2 >= nextC && nextC <= lastC) {
                // two chroma rows of every layer in one instruction
                const uint32_t slot = (uint32_t)(2 * NL * ST_YL + (((nextC - baseC) >> 1) & 1) * (NL * CLB));
                const int r = min(max(nextC + rrC, 0), SC.h - 1);
                const size_t roff = (size_t)r * SC.pitch + (size_t)colC;
                const int li = liC;
                const bool act = li < NL && vecC < nvecC && nextC + rrC <= lastC;
                const uint8_t *pl = li == 0 ? planeC[0] : li == 1 ? planeC[NL > 1 ? 1 : 0] : li == 2 ? planeC[NL > 2 ? 2 : 0] : planeC[NL > 3 ? 3 : 0];
                st_dma(pl + roff, act, lds0 + slot);
                if constexpr (PL) {
                    // the V planes (the shape of the U planes, host-checked) into the region behind the U rows
                    const uint8_t *pv = li == 0 ? planeV[0] : li == 1 ? planeV[NL > 1 ? 1 : 0] : li == 2 ? planeV[NL > 2 ? 2 : 0] : planeV[NL > 3 ? 3 : 0];
                    st_dma(pv + roff, act, lds0 + slot + (uint32_t)(2 * NL * ST_CLP));
                    issued += 1;
                }
                nextC += 2; issued += 1; seqC = issued;
            }
            // (first row of a chunk, rows skipped by a strong reduction: what was just requested is needed now)
            if (ry + 1 >= landY || rc + 1 >= landC) { await(0); landY = nextY; landC = nextC; }
            }
        }
        // The previous row's pixels are stored HERE, right after this row's wait: gfx950 has one counter for loads and stores, the wait above
        // drains it, and a store issued just before it would be waited for every time (a write latency per wait); issued now it has
        // until the next wait, a row or two away.
        if (j > 0 && x < T.W && !(CHV_ST_ABL & 2)) st_store(D.ptr + (size_t)(y0 + j - 1) * D.pitch, (uint32_t)x * 4u, pending);
        // ---- tap addresses and weights, once for all layers -----------------------------------------------------------------
        auto yoff = [&](int q) { return ((q >> 2) & 1) * (NL * ST_YL) + (q & 3) * ST_PITCH; };                       // layer 0's copy of luma row baseY + q
        auto coff = [&](int q) { return 2 * NL * ST_YL + ((q >> 1) & 1) * (NL * CLB) + (q & 1) * CPITCH; };
        const int sY0 = yoff(ry - baseY), sY1 = yoff(ry + 1 - baseY), sC0 = coff(rc - baseC), sC1 = coff(rc + 1 - baseC);
        // LDS byte addresses of layer 0's taps: the rings' address and the row's slot are added on the scalar unit, the lane's column once per tap
        const uint32_t bY0 = lds0 + (uint32_t)sY0, bY1 = lds0 + (uint32_t)sY1, bC0 = lds0 + (uint32_t)sC0, bC1 = lds0 + (uint32_t)sC1;
        const uint32_t aY00 = bY0 + (uint32_t)oy0, aY10 = bY0 + (uint32_t)oy1, aY01 = bY1 + (uint32_t)oy0, aY11 = bY1 + (uint32_t)oy1;
        const uint32_t aC00 = bC0 + (uint32_t)oc0v, aC10 = bC0 + (uint32_t)oc1v, aC01 = bC1 + (uint32_t)oc0v, aC11 = bC1 + (uint32_t)oc1v;
        const float iyb = __uint_as_float(re.z), icb = __uint_as_float(re.w);
        const float w00 = iya * iyb, w10 = ya * iyb, w01 = iya * yb, w11 = ya * yb;
        const float c00 = ica * icb, c10 = ca * icb, c01 = ica * cbw, c11 = ca * cbw;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;                          // img_clear_bgra: (0, 0, 0, 1) — the canvas pixel as float codes
        [[maybe_unused]] int32_t q0 = 0, q1 = 0, q2 = 0;             // OPQ: the bottom layer's pixel, clamped 16.16 sums
        if constexpr (CRY) {
            // ---- the carried chroma: read what is new to the lane, where the transient form reads its taps (behind the ring's await) ----
            // Tap rows rc (weights c00, c10) and rc + 1 (c01, c11): rc lies in the set of its parity, rc + 1 in the other.  Advance 0 reads
            // nothing, advance 1 one set, the chunk's first row and any larger advance both.  The registers hold bytes, not ring slots: a
            // ring request may overwrite a row the lane still carries (the `s_waitcnt lgkmcnt(0)` in front of a request has seen the reads).
            // (the weights in FRONT of the reads: hipcc's own wait for the row entry they are made of is a full `lgkmcnt(0)`, and behind the
            // reads it would sit out their round trip before the first multiply — 0.5 % of the launch)
            asm volatile("" :: "v"(w00), "v"(w10), "v"(w01), "v"(w11), "v"(c00), "v"(c10), "v"(c01), "v"(c11));
            const int par = (rc - baseC) & 1;
            const int row0 = rc + par, row1 = rc + 1 - par;
            if (held0 != row0) {
                const uint32_t bc = lds0 + (uint32_t)coff(row0 - baseC);
                st_carry_read<NL>(cset[0], bc + (uint32_t)oc0v, bc + (uint32_t)oc1v);
                held0 = row0;
            }
            if (held1 != row1) {
                const uint32_t bc = lds0 + (uint32_t)coff(row1 - baseC);
                st_carry_read<NL>(cset[1], bc + (uint32_t)oc0v, bc + (uint32_t)oc1v);
                held1 = row1;
            }
            // luma as in the transient form: one wait per layer, the next layer's four taps in flight under this layer's arithmetic
            // (layer 0's wait stands in FRONT of the branch below and covers the row's chroma groups: inside the two copies the carried
            // registers are only read — redefined there, each would need a copy where the two paths join, and a copy of a register whose
            // read is still in flight copies the old byte)
            StLuma lum[2];
            st_luma_read<0>(lum[0], aY00, aY10, aY01, aY11);
            st_carry_wait<NL, 0>(lum[0], cset[0], cset[1]);
            // The reference accumulates top-left, top-right, bottom-left, bottom-right: which set is the top row is the parity, and a select
            // per byte would cost what the reads saved — the rest of the row exists twice, chosen by one uniform branch (pack and select
            // included: only `pending` joins).
            auto rest = [&](auto top_even) {
                constexpr int TOP = decltype(top_even)::value ? 0 : 1;
                auto clayer = [&](auto lt) {
                    constexpr int l = decltype(lt)::value;
                    if constexpr (l < NL) {
                        // (every register a copy reads by hand is read AND awaited inside the copy: the next layer's luma taps)
                        if constexpr (l + 1 < NL) st_luma_read<(l + 1) * ST_YL>(lum[(l + 1) & 1], aY00, aY10, aY01, aY11);
                        if constexpr (l >= 1 && l + 1 < NL) st_luma_wait<4>(lum[l & 1]);
                        else if constexpr (l >= 1) st_luma_wait<0>(lum[l & 1]);
                        const StLuma &t = lum[l & 1];
                        const uint32_t *ct = cset[TOP].c[l], *cb_ = cset[1 - TOP].c[l];
                        int32_t cb, cg, cr;
                        if constexpr (DN) {
                            // (the registers the byte reads filled ARE the operands: b x 2^-149; fy, fu, fv are the samples x 2^-22)
                            const float fy = cs_mix_d(w00, w10, w01, w11, t.y00, t.y10, t.y01, t.y11);
                            const float fu = cs_mix_d(c00, c10, c01, c11, ct[0], ct[1], cb_[0], cb_[1]);
                            const float fv = cs_mix_d(c00, c10, c01, c11, ct[2], ct[3], cb_[2], cb_[3]);
                            yuv_to_bgr_fixed_absorbed_d(csc[l], unscale, fy, fu, fv, cb, cg, cr);
                        } else {
                        const float fy = cs_mix_h(w00, w10, w01, w11, tap_h(t.y00), tap_h(t.y10), tap_h(t.y01), tap_h(t.y11));
                        const float fu = cs_mix_h(c00, c10, c01, c11, tap_h(ct[0]), tap_h(ct[1]), tap_h(cb_[0]), tap_h(cb_[1]));
                        const float fv = cs_mix_h(c00, c10, c01, c11, tap_h(ct[2]), tap_h(ct[3]), tap_h(cb_[2]), tap_h(cb_[3]));
                        yuv_to_bgr_fixed_absorbed(csc[l], fy, fu, fv, cb, cg, cr);
                        }
                        const float a24 = al24[l];
                        if constexpr (l == 0) {
                            q0 = cb; q1 = cg; q2 = cr;
                            return;
                        } else if constexpr (l == 1) {
                            r0 = __builtin_fmaf(a24, (float)code_h(cb), __builtin_fmaf(ial24, (float)code_h(q0), 0.0f));
                            r1 = __builtin_fmaf(a24, (float)code_h(cg), __builtin_fmaf(ial24, (float)code_h(q1), 0.0f));
                            r2 = __builtin_fmaf(a24, (float)code_h(cr), __builtin_fmaf(ial24, (float)code_h(q2), 0.0f));
                        } else {
                            r0 = __builtin_fmaf(a24, (float)code_h(cb), __builtin_fmaf(r0, ial[l], nrb[l]));
                            r1 = __builtin_fmaf(a24, (float)code_h(cg), __builtin_fmaf(r1, ial[l], nrb[l]));
                            r2 = __builtin_fmaf(a24, (float)code_h(cr), __builtin_fmaf(r2, ial[l], nrb[l]));
                        }
                        if (l + 1 < NL) { r0 += kRintBias; r1 += kRintBias; r2 += kRintBias; }
                    }
                };
                clayer(std::integral_constant<int, 0>{}); clayer(std::integral_constant<int, 1>{}); clayer(std::integral_constant<int, 2>{}); clayer(std::integral_constant<int, 3>{});
                uint32_t out;
                asm("v_cvt_pk_u8_f32 %0, %1, 0, %2" : "=v"(out) : "v"(r0), "v"(alpha_word));
                asm("v_cvt_pk_u8_f32 %0, %1, 1, %0" : "+v"(out) : "v"(r1));
                asm("v_cvt_pk_u8_f32 %0, %1, 2, %0" : "+v"(out) : "v"(r2));
                pending = (lane_pic && row_pic) ? out : alpha_word;
            };
            if (par) rest(std::false_type{}); else rest(std::true_type{});
            continue;
        }
        // One wait per layer, and the next layer's taps in flight under this layer's arithmetic (a group belongs to the CURRENT row: nothing is
        // read across rows, so the `s_waitcnt lgkmcnt(0)` in front of a ring request still means "the rows being overwritten have been read")
        // (planar sources keep three more plane pointers per layer set and the V offsets: the twelve registers of a second group do not fit
        // 80 there without scratch — each layer's group is read and awaited on its own, still one wait per layer)
        constexpr bool AHEAD = !PL;
        StTaps taps[2];
        auto read_layer = [&](auto lt) {
            constexpr int l = decltype(lt)::value;
            st_taps_read<l * ST_YL, l * CLB, l * CLB + VOFF>(taps[l & 1], aY00, aY10, aY01, aY11, aC00, aC10, aC01, aC11);
        };
        if (!(CHV_ST_ABL & 4)) read_layer(std::integral_constant<int, 0>{});
        auto layer = [&](auto lt) {
            constexpr int l = decltype(lt)::value;
            if constexpr (l < NL && !(CHV_ST_ABL & 4)) {
            if constexpr (l + 1 < NL && AHEAD) { read_layer(std::integral_constant<int, l + 1>{}); st_taps_wait<12>(taps[l & 1]); }
            else {
                if constexpr (l > 0 && !AHEAD) read_layer(lt);
                st_taps_wait<0>(taps[l & 1]);
            }
            const StTaps &t = taps[l & 1];
            const float fy = cs_mix_h(w00, w10, w01, w11, tap_h(t.y00), tap_h(t.y10), tap_h(t.y01), tap_h(t.y11));
            const float fu = cs_mix_h(c00, c10, c01, c11, tap_h(t.u00), tap_h(t.u10), tap_h(t.u01), tap_h(t.u11));
            const float fv = cs_mix_h(c00, c10, c01, c11, tap_h(t.v00), tap_h(t.v10), tap_h(t.v01), tap_h(t.v11));
            if constexpr (ABS && CHV_STREAM_PMIX) {
                // the layer's pixel enters the blend as a binary16 read from the high half of its clamped 16.16 sum (code x 2^-24, exact;
                // the opacity carries the 2^24): p * a + inner in one v_fma_mix_f32, the same real numbers into the same single rounding
                int32_t cb, cg, cr;
                yuv_to_bgr_fixed_absorbed(csc[l], fy, fu, fv, cb, cg, cr);
                const float a24 = al24[l];
                if constexpr (OPQ && l == 0) {
                    q0 = cb; q1 = cg; q2 = cr;                       // opacity 1 on the cleared canvas: the pixel is the layer's code
                    return;
                } else if constexpr (OPQ && l == 1) {
                    r0 = __builtin_fmaf(a24, (float)code_h(cb), __builtin_fmaf(ial24, (float)code_h(q0), 0.0f));
                    r1 = __builtin_fmaf(a24, (float)code_h(cg), __builtin_fmaf(ial24, (float)code_h(q1), 0.0f));
                    r2 = __builtin_fmaf(a24, (float)code_h(cr), __builtin_fmaf(ial24, (float)code_h(q2), 0.0f));
                } else if (l == 0) {
                    r0 = __builtin_fmaf(a24, (float)code_h(cb), 0.0f); r1 = __builtin_fmaf(a24, (float)code_h(cg), 0.0f); r2 = __builtin_fmaf(a24, (float)code_h(cr), 0.0f);
                } else {
                    r0 = __builtin_fmaf(a24, (float)code_h(cb), __builtin_fmaf(r0, ial[l], nrb[l]));
                    r1 = __builtin_fmaf(a24, (float)code_h(cg), __builtin_fmaf(r1, ial[l], nrb[l]));
                    r2 = __builtin_fmaf(a24, (float)code_h(cr), __builtin_fmaf(r2, ial[l], nrb[l]));
                }
                if (l + 1 < NL) { r0 += kRintBias; r1 += kRintBias; r2 += kRintBias; }
                return;
            }
            float pb, pg, pr;
            if constexpr (ABS) yuv_to_bgr_floats_absorbed(csc[l], fy, fu, fv, pb, pg, pr);
            else yuv_to_bgr_floats(csc[l], (int)code_biased(fy), (int)code_biased(fu), (int)code_biased(fv), pb, pg, pr);
            if (l == 0) {                // the cleared canvas: fma(p, a, 0 * (1 - a)) = RN(p * a) for a in [0, 1]
                r0 = pb * al[0]; r1 = pg * al[0]; r2 = pr * al[0];
            } else {                     // (r holds 2^23 + the codes the previous layer's store would have kept: see nrb above)
                r0 = __builtin_fmaf(pb, al[l], __builtin_fmaf(r0, ial[l], nrb[l]));
                r1 = __builtin_fmaf(pg, al[l], __builtin_fmaf(r1, ial[l], nrb[l]));
                r2 = __builtin_fmaf(pr, al[l], __builtin_fmaf(r2, ial[l], nrb[l]));
            }
            if (l + 1 < NL) { r0 += kRintBias; r1 += kRintBias; r2 += kRintBias; }
            }
        };
        layer(std::integral_constant<int, 0>{}); layer(std::integral_constant<int, 1>{}); layer(std::integral_constant<int, 2>{}); layer(std::integral_constant<int, 3>{});
        // (pack_codes with the alpha word as a separate source: tied to the destination it is re-materialised every row)
        uint32_t out;
        asm("v_cvt_pk_u8_f32 %0, %1, 0, %2" : "=v"(out) : "v"(r0), "v"(alpha_word));
        asm("v_cvt_pk_u8_f32 %0, %1, 1, %0" : "+v"(out) : "v"(r1));
        asm("v_cvt_pk_u8_f32 %0, %1, 2, %0" : "+v"(out) : "v"(r2));
        // a pixel outside the picture keeps the cleared canvas (inside the border quad its alpha is forced: the same word)
        const uint32_t res = (lane_pic && row_pic) ? out : alpha_word;
        pending = res;
    }
    if (nrows > 0 && x < T.W && !(CHV_ST_ABL & 2)) st_store(D.ptr + (size_t)(y0 + nrows - 1) * D.pitch, (uint32_t)x * 4u, pending);
}

// one tick, descriptors by value (96 + NL x 368 bytes of kernel arguments)
template <int NL>
struct StreamOne {
    DTick t;
    DLayer l[NL];
};

}  // namespace chv
