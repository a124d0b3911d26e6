// tests/cpp/test_stream_plan.cpp — stream_plan.h on the CPU: the planner of tick_bgra_stream's launches and the decode its kernels run, over
// every (block, wave) of every plan.  Built and run by tests/test_stream_plan.py (also, on fewer batches, with -fsanitize=address,undefined); exit status 0 =
// every expectation held, else 1 with the first failure on stderr.
#include "stream_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace chv;

static const int WAVES = 4;       // strips per block (ST_WAVES)

#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s — ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// launch_bgra_stream's rule before there were plans, restated: 1024 SIMDs x 6 waves x 12 rounds; small launches 4 .. 12 rows for 4 800 waves
static int todays_rows(int n_ticks, int strips_x, int maxH, int forced) {
    const long want = 1024L * 6 * 12;
    long chunks = want / ((long)n_ticks * strips_x > 1 ? (long)n_ticks * strips_x : 1);
    if (chunks < 1) chunks = 1;
    const long wave_rows = (long)n_ticks * strips_x * maxH;
    long rows_small = (wave_rows + 4800 - 1) / 4800;
    if (rows_small < 4) rows_small = 4;
    if (rows_small > 12) rows_small = 12;
    long rows = (maxH + chunks - 1) / chunks;
    if (rows < rows_small) rows = rows_small;
    if (forced) rows = forced;
    if (rows > maxH) rows = maxH;
    if (rows < 1) rows = 1;
    return (int)rows;
}
// today's block -> (tick, chunk, strip), restated
static bool todays_map(int n_ticks, int strips_x, int chunks_y, int b, int wave, int &tick, int &chunk, int &strip) {
    const int groups_x = (strips_x + WAVES - 1) / WAVES;
    const int total = n_ticks * chunks_y * groups_x;
    const int per_xcd = (total + 7) >> 3;
    const int idx = (b & 7) * per_xcd + (b >> 3);
    if ((b >> 3) >= per_xcd || idx >= total) return false;
    tick = idx / (chunks_y * groups_x);
    const int rem = idx - tick * (chunks_y * groups_x);
    chunk = rem / groups_x;
    strip = (rem - chunk * groups_x) * WAVES + wave;
    return strip < strips_x;
}

static long g_plans = 0, g_phased = 0;

static void check(int n_ticks, int strips_x, int maxH, long slots, int forced, int tenths, int tall, int den) {
    StreamRowsRule rule{ 1024L * 6 * 12, 4800, 12, 4, 0, forced };
    StreamPlanShape shape{ tall, den, 24, tenths };
    const StreamPlan p = stream_plan_make(n_ticks, strips_x, maxH, slots, false, rule, shape, WAVES);
    const int n_phase = stream_plan_phases(p);
    g_plans++;
    g_phased += n_phase > 1;
    EXPECT(n_phase >= 1 && n_phase <= 4, "%d phases", n_phase);
    if (forced) EXPECT(n_phase == 1, "a forced height gave %d phases", n_phase);
    // the gate: a phased plan's tall phase alone holds tenths / 10 rounds of the slots, and is taller than the uniform rule's chunks
    if (n_phase > 1) {
        const long tall_waves = (long)p.ph[0].n_ticks * strips_x * p.ph[0].chunks_y;
        EXPECT(tall_waves * 10 >= (long)tenths * slots, "%d ticks x %d strips x %d rows, %ld slots: a tall phase of %ld waves", n_ticks, strips_x, maxH, slots, tall_waves);
        EXPECT(p.ph[0].rows > todays_rows(n_ticks, strips_x, maxH, 0) && p.ph[0].rows <= (tall < maxH ? tall : maxH), "a tall phase of %d rows", p.ph[0].rows);
    }
    // per-tick heights: the tallest is maxH, others are smaller
    std::vector<int> H(n_ticks);
    for (int t = 0; t < n_ticks; t++) H[t] = t % 3 == 1 ? (maxH + 1) / 2 : t % 5 == 4 ? (maxH > 7 ? maxH - 7 : 1) : maxH;
    long blocks = 0;
    int next_tick = 0;
    for (int k = 0; k < kStreamPhases; k++) {
        const StreamPhase &q = p.ph[k];
        if (k >= n_phase) { EXPECT(q.first_block == kStreamNoPhase && q.n_ticks == 0, "phase %d is not empty", k); continue; }
        EXPECT(q.first_block == blocks && q.first_block % 8 == 0, "phase %d begins at block %d, expected %ld", k, q.first_block, blocks);
        EXPECT(q.first_tick == next_tick && q.n_ticks >= 1, "phase %d: ticks from %d (%d of them), expected from %d", k, q.first_tick, q.n_ticks, next_tick);
        EXPECT(q.rows >= 1 && q.rows <= maxH && q.chunks_y == (maxH + q.rows - 1) / q.rows, "phase %d: %d chunks of %d rows for %d", k, q.chunks_y, q.rows, maxH);
        if (k > 0) EXPECT(q.rows <= p.ph[k - 1].rows, "phase %d is taller (%d) than the one before (%d)", k, q.rows, p.ph[k - 1].rows);
        if (n_phase > 1 && k == n_phase - 1 && maxH >= 48) EXPECT(q.rows >= 24, "the last phase has %d rows", q.rows);
        blocks += stream_phase_blocks(q, strips_x, WAVES);
        next_tick += q.n_ticks;
    }
    EXPECT(next_tick == n_ticks, "%d of %d ticks planned", next_tick, n_ticks);
    EXPECT(blocks == stream_plan_blocks(p, strips_x, WAVES), "grid %ld, phases sum to %ld", stream_plan_blocks(p, strips_x, WAVES), blocks);
    if (n_phase == 1) EXPECT(p.ph[0].rows == todays_rows(n_ticks, strips_x, maxH, forced), "one phase of %d rows, today's rule says %d", p.ph[0].rows, todays_rows(n_ticks, strips_x, maxH, forced));
    // every (tick, strip, canvas row) exactly once
    std::vector<unsigned char> seen((size_t)n_ticks * strips_x * maxH, 0);
    for (long b = 0; b < blocks; b++)
        for (int wave = 0; wave < WAVES; wave++) {
            int tick = -1, y0 = -1, rows = -1, strip = -1;
            const bool work = stream_plan_decode(p, strips_x, WAVES, (int)b, wave, tick, y0, rows, strip);
            if (n_phase == 1) {
                int t2 = -1, c2 = -1, s2 = -1;
                const bool w2 = todays_map(n_ticks, strips_x, p.ph[0].chunks_y, (int)b, wave, t2, c2, s2);
                EXPECT(work == w2 && (!work || (tick == t2 && y0 == c2 * p.ph[0].rows && strip == s2 && rows == p.ph[0].rows)), "block %ld wave %d differs from today's map", b, wave);
            }
            if (!work) continue;
            EXPECT(tick >= 0 && tick < n_ticks && strip >= 0 && strip < strips_x && y0 >= 0 && rows >= 1, "block %ld wave %d -> tick %d strip %d y0 %d rows %d", b, wave, tick, strip, y0, rows);
            // (the kernel: chunks below a shorter tick return; the others run min(rows, H - y0) rows)
            if (y0 >= H[tick]) continue;
            const int nrows = rows < H[tick] - y0 ? rows : H[tick] - y0;
            for (int y = y0; y < y0 + nrows; y++) {
                unsigned char &s = seen[((size_t)tick * strips_x + strip) * maxH + y];
                EXPECT(!s, "tick %d strip %d row %d covered twice (block %ld)", tick, strip, y, b);
                s = 1;
            }
        }
    for (int t = 0; t < n_ticks; t++)
        for (int s = 0; s < strips_x; s++)
            for (int y = 0; y < maxH; y++)
                EXPECT(seen[((size_t)t * strips_x + s) * maxH + y] == (y < H[t] ? 1 : 0), "tick %d strip %d row %d: covered %d times", t, s, y, seen[((size_t)t * strips_x + s) * maxH + y]);
}

int main(int argc, char **) {
    const bool quick = argc > 1;         // (any argument: a third of the batches — the sanitizer build's run)
    const int heights[] = { 1, 23, 24, 52, 96, 719, 720, 1080 };
    const long slots[] = { 8, 64, 5120, 6144 };
    const int talls[] = { 720, 360, 240, 120 };
    std::vector<int> ticks;
    for (int n = 1; n <= 40; n++) ticks.push_back(n);
    ticks.push_back(255); ticks.push_back(256); ticks.push_back(257);
    for (int n : ticks)
        for (int sx = 1; sx <= 21; sx++) {
            if (quick && n > 12 && n != 256) continue;
            for (int h : heights)
                for (long sl : slots) {
                    const int variant = (n + sx + h) % 4;
                    check(n, sx, h, sl, 0, sl <= 64 ? 1 : 20, talls[variant], variant & 1 ? 4 : 8);
                }
            check(n, sx, 720, 6144, 52, 20, 240, 8);           // a forced CHV_STREAM_ROWS: one phase
            check(n, sx, 96, 8, 33, 1, 240, 8);
        }
    // the headline: 256 ticks of 1280 x 720 -> a tall phase and three closing ones
    {
        StreamRowsRule rule{ 1024L * 6 * 12, 4800, 12, 4, 0, 0 };
        const StreamPlan p = stream_plan_make(256, 20, 720, 6144, false, rule, StreamPlanShape{ 240, 8, 24, 20 }, WAVES);
        EXPECT(stream_plan_phases(p) == 4 && p.ph[0].rows == 240 && p.ph[0].n_ticks == 224 && p.ph[1].rows == 120 && p.ph[2].rows == 60 && p.ph[3].rows == 30,
               "%d phases, %d rows over %d ticks first", stream_plan_phases(p), p.ph[0].rows, p.ph[0].n_ticks);
        // off, the by-value lone tick and a batch whose tall phase would not fill the chip: today's single phase
        EXPECT(stream_plan_phases(stream_plan_make(256, 20, 720, 6144, false, rule, StreamPlanShape{ 0, 8, 24, 20 }, WAVES)) == 1, "shape.tall == 0 phased");
        EXPECT(stream_plan_make(256, 20, 720, 6144, false, rule, StreamPlanShape{ 0, 8, 24, 20 }, WAVES).ph[0].rows == 52, "the headline's uniform height");
        EXPECT(stream_plan_phases(stream_plan_make(1, 20, 720, 8, true, rule, StreamPlanShape{ 240, 8, 24, 1 }, WAVES)) == 1, "the by-value lone tick phased");
        EXPECT(stream_plan_phases(stream_plan_make(16, 20, 720, 6144, false, rule, StreamPlanShape{ 240, 8, 24, 20 }, WAVES)) == 1, "sixteen ticks phased");
    }
    // batches whose tall phase would not fill the chip once: a smaller tall height, or the uniform rule (5 120 slots: the five-wave kernels)
    {
        StreamRowsRule rule{ 1024L * 6 * 12, 4800, 12, 4, 0, 0 };
        const StreamPlanShape shape{ 240, 4, 24, 10 };
        struct { int n, sx, h, phases, tall; } want[] = { { 21, 20, 720, 1, 12 }, { 24, 20, 720, 1, 12 }, { 32, 20, 720, 2, 60 }, { 48, 20, 720, 2, 60 }, { 64, 20, 720, 3, 120 },
                                                          { 96, 20, 720, 3, 120 }, { 128, 20, 720, 4, 240 }, { 256, 20, 720, 4, 240 }, { 10, 30, 1080, 1, 12 },
                                                          { 64, 30, 1080, 4, 216 }, { 3, 60, 2160, 1, 12 } };
        for (const auto &w : want) {
            const StreamPlan p = stream_plan_make(w.n, w.sx, w.h, 5120, false, rule, shape, WAVES);
            EXPECT(stream_plan_phases(p) == w.phases && p.ph[0].rows == w.tall, "%d ticks of %d rows: %d phases, %d rows first", w.n, w.h, stream_plan_phases(p), p.ph[0].rows);
        }
    }
    EXPECT(g_phased > 500 && g_plans - g_phased > 500, "%ld plans, %ld phased", g_plans, g_phased);
    printf("%ld plans, %ld of them phased\n", g_plans, g_phased);
    return 0;
}
