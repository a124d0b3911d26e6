// stream_plan.h — how a batch launch of tick_bgra_stream is cut into waves: up to four PHASES, each a uniform grid of chunks over a contiguous
// range of the batch's ticks, tall chunks first and short ones at the end (launch_bgra_stream plans, stream_body decodes; no HIP in here:
// tests/cpp/test_stream_plan.cpp runs both on the CPU).
//
// Every chunk pays a fixed part — the column setup, the chunk's last tap rows, a first ring fill awaited in full, the rest of its last row
// table, the overshoot rows the chunk above fetched as well — that tall chunks amortise, and a launch of few tall chunks pays at its end,
// where the last waves finish alone.  A launch whose first waves are tall and whose last waves are short has both: blocks are dispatched in
// index order, so phase 0 runs first and the last phase ends the launch.
#pragma once

#if defined(__HIPCC__)
#define CHV_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define CHV_HOST_DEVICE inline
#endif

namespace chv {

constexpr int kStreamPhases = 4;
constexpr int kStreamNoPhase = 0x7FFFFFFF;       // first_block of an unused phase: no block index reaches it

// blocks [first_block, first_block + 8 * ceil(n_ticks * chunks_y * groups_x / 8)) work on ticks [first_tick, first_tick + n_ticks) in chunks of `rows`
// canvas rows, chunks_y of them per tick
struct StreamPhase {
    int first_block, first_tick, n_ticks, chunks_y, rows;
};
// 80 bytes: a kernel argument, read as scalar loads at constant offsets.  Phases in use come first, first_block rising (each a multiple of
// 8: block b stays on XCD b % 8); unused ones have first_block = kStreamNoPhase and no ticks.
struct StreamPlan {
    StreamPhase ph[kStreamPhases];
};
static_assert(sizeof(StreamPlan) <= 80, "the plan is a kernel argument");

inline int stream_plan_phases(const StreamPlan &p) {
    int n = 0;
    while (n < kStreamPhases && p.ph[n].n_ticks > 0) n++;
    return n;
}
// blocks of one phase: its (tick, chunk, group of `waves` strips) triples, rounded up to the eight XCDs
inline long stream_phase_blocks(const StreamPhase &q, int strips_x, int waves) {
    const long total = (long)q.n_ticks * q.chunks_y * ((strips_x + waves - 1) / waves);
    return ((total + 7) / 8) * 8;
}
inline long stream_plan_blocks(const StreamPlan &p, int strips_x, int waves) {
    long n = 0;
    for (int k = 0; k < stream_plan_phases(p); k++) n += stream_phase_blocks(p.ph[k], strips_x, waves);
    return n;
}

// What wave `wave` of block `b` (counted from the phase's first block) does inside ONE phase: false = nothing.  XCD-aware numbering: block b
// runs on XCD b % 8, and an XCD owns a contiguous range of (tick, chunk, group of `waves` strips).  y0 may lie below a tick that is shorter
// than the launch's tallest: the caller holds the tick and drops those.
CHV_HOST_DEVICE bool stream_phase_decode(int first_tick, int n_ticks, int chunks_y, int rows, int strips_x, int waves, int b, int wave, int &tick, int &y0, int &strip) {
    const int groups_x = (strips_x + waves - 1) / waves;
    const int total = n_ticks * chunks_y * groups_x;
    const int per_xcd = (total + 7) >> 3;
    const int idx = (b & 7) * per_xcd + (b >> 3);
    if ((b >> 3) >= per_xcd || idx >= total) return false;
    const int t = idx / (chunks_y * groups_x), rem = idx - t * (chunks_y * groups_x);
    const int chunk = rem / groups_x;
    strip = (rem - chunk * groups_x) * waves + wave;
    if (strip >= strips_x) return false;
    tick = first_tick + t;
    y0 = chunk * rows;
    return true;
}

// The same for a plan: the block's phase by at most three compares (unused phases begin at kStreamNoPhase), then the phase's own numbering.
// `rows`: the phase's chunk height (the wave's rows: min(rows, the tick's H - y0)).
CHV_HOST_DEVICE bool stream_plan_decode(const StreamPlan &p, int strips_x, int waves, int block, int wave, int &tick, int &y0, int &rows, int &strip) {
    // (field by field: a selected copy of a whole phase would keep the argument in private memory on the device)
    const bool k1 = block >= p.ph[1].first_block, k2 = block >= p.ph[2].first_block, k3 = block >= p.ph[3].first_block;
#define CHV_PLAN_FIELD(f) (k3 ? p.ph[3].f : k2 ? p.ph[2].f : k1 ? p.ph[1].f : p.ph[0].f)
    const int first_block = CHV_PLAN_FIELD(first_block), first_tick = CHV_PLAN_FIELD(first_tick), n_ticks = CHV_PLAN_FIELD(n_ticks);
    const int chunks_y = CHV_PLAN_FIELD(chunks_y);
    rows = CHV_PLAN_FIELD(rows);
#undef CHV_PLAN_FIELD
    return stream_phase_decode(first_tick, n_ticks, chunks_y, rows, strips_x, waves, block - first_block, wave, tick, y0, strip);
}

// ---------------------------------------------------------------------------------------------------------------------
// the planner (host)
// ---------------------------------------------------------------------------------------------------------------------
// the uniform rule (one height for the whole launch), as launch_bgra_stream has kept it since the kernel had one strip per block
struct StreamRowsRule {
    long want_waves;            // waves a launch that fills the chip is cut into: SIMDs x waves per SIMD x rounds
    long small_waves;           // waves a small launch is cut into ...
    int small_rows_max;         // ... in chunks of at most this many rows
    int min_rows;
    int rows_fixed;             // > 0: a build's fixed height (sweeps)
    int rows_forced;            // > 0: CHV_STREAM_ROWS (tests)
};
inline int stream_uniform_rows(const StreamRowsRule &r, int n_ticks, int strips_x, int maxH) {
    const long strips = (long)n_ticks * strips_x > 1 ? (long)n_ticks * strips_x : 1;
    const long chunks = r.want_waves / strips > 1 ? r.want_waves / strips : 1;
    const long wave_rows = (long)n_ticks * strips_x * maxH;
    long rows_small = (wave_rows + r.small_waves - 1) / r.small_waves;
    if (rows_small < r.min_rows) rows_small = r.min_rows;
    if (rows_small > r.small_rows_max) rows_small = r.small_rows_max;
    long rows = (maxH + chunks - 1) / chunks;
    if (rows < rows_small) rows = rows_small;
    if (r.rows_fixed > 0) rows = r.rows_fixed;
    if (r.rows_forced > 0) rows = r.rows_forced;
    if (rows > maxH) rows = maxH;
    if (rows < 1) rows = 1;
    return (int)rows;
}

// the phased form: a tall first phase over most ticks, then up to three closing phases over the last ticks whose heights fall by half
struct StreamPlanShape {
    int tall;                   // rows per chunk of the first phase (cut to the canvas); 0: never phase
    int closing_den;            // 1 / closing_den of the ticks go to the closing phases (at least one tick per closing phase)
    int shortest;               // no closing phase is cut shorter than this
    int tall_tenths;            // the gate: the tall phase alone holds at least tall_tenths / 10 rounds of the chip's wave slots
};

inline StreamPlan stream_plan_single(int n_ticks, int maxH, int rows) {
    StreamPlan p;
    for (int k = 0; k < kStreamPhases; k++) p.ph[k] = StreamPhase{ kStreamNoPhase, 0, 0, 1, 1 };
    rows = rows < 1 ? 1 : rows > maxH && maxH >= 1 ? maxH : rows;
    p.ph[0] = StreamPhase{ 0, 0, n_ticks, (maxH + rows - 1) / rows, rows };
    return p;
}

// `slots`: waves the chip holds at once — SIMDs x the launched kernel's waves per SIMD; `by_value`: the lone tick whose descriptors are
// kernel arguments (its kernels take no plan).
// The gate counts the PLAN's own waves: a wave's rows are a serial chain, and tall chunks pay only where other waves fill the SIMD meanwhile
// — the tall phase alone must hold shape.tall_tenths / 10 rounds of `slots`.  A batch too small for that at the shape's tall height is tried
// at half of it, and again, while a closing phase still fits above `shortest`; then it keeps the uniform rule.
inline StreamPlan stream_plan_make(int n_ticks, int strips_x, int maxH, long slots, bool by_value, const StreamRowsRule &rule, const StreamPlanShape &shape, int waves) {
    const int rows_u = stream_uniform_rows(rule, n_ticks, strips_x, maxH);
    const StreamPlan single = stream_plan_single(n_ticks, maxH, rows_u);
    if (by_value || rule.rows_fixed > 0 || rule.rows_forced > 0 || shape.tall <= 0 || n_ticks < 2 || slots < 1) return single;
    // equal chunks inside a phase: the height that cuts the canvas into as many chunks as `h` would
    auto even = [&](int h) { const int c = (maxH + h - 1) / h; return (maxH + c - 1) / c; };
    for (int want = shape.tall < maxH ? shape.tall : maxH; want >= 2 * shape.shortest && want >= 2; want /= 2) {
        const int tall = even(want);
        if (tall <= rows_u) break;
        int heights[kStreamPhases] = { tall, 0, 0, 0 }, n_phase = 1;
        for (int h = tall / 2; n_phase < kStreamPhases && n_phase < n_ticks && h >= shape.shortest && h >= 1; h /= 2) {
            const int e = even(h);
            if (e >= heights[n_phase - 1]) break;
            heights[n_phase++] = e;
        }
        if (n_phase < 2) break;
        const int n_close = n_phase - 1;
        int closing = shape.closing_den > 0 ? n_ticks / shape.closing_den : 0;
        if (closing < n_close) closing = n_close;
        if (closing > n_ticks - 1) closing = n_ticks - 1;
        const long tall_waves = (long)(n_ticks - closing) * strips_x * ((maxH + tall - 1) / tall);
        if (tall_waves * 10 < (long)shape.tall_tenths * slots) continue;
        StreamPlan p = single;
        int tick = 0;
        long block = 0;
        for (int k = 0; k < n_phase; k++) {
            // the closing ticks in equal shares, the remainder to the taller phases
            const int nt = k == 0 ? n_ticks - closing : closing / n_close + (k - 1 < closing % n_close ? 1 : 0);
            p.ph[k] = StreamPhase{ (int)block, tick, nt, (maxH + heights[k] - 1) / heights[k], heights[k] };
            tick += nt;
            block += stream_phase_blocks(p.ph[k], strips_x, waves);
        }
        return p;
    }
    return single;
}

}  // namespace chv
