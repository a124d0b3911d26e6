// kernels_stream.hip.cpp — tick_bgra_stream: ticks of 1..4 full-frame NV12 (or, all of them, y420p) video layers of ONE geometry onto a cleared BGRA canvas
// (the bench headline's tick, cfg2's tick; VideoMixer.mix of N camera feeds scaled to the canvas, mix.video.swift:114-124), rows
// outermost and the layers innermost.
//
// tick_bgra_wave (kernels_wave.hip.cpp) stages one layer's rectangle for a 64 x 16 strip (6.7 KB), runs the rows of that layer,
// stages the next one: the eight weight products of a pixel row, its row-table reads and the canvas pixel's trip through packed
// codes are paid once per row AND layer, because four rectangles do not fit beside each other at five waves per SIMD
// (profiles/r03_notes.md section 7).  Here nothing is staged as a rectangle.  A wave owns a 64-column strip of the canvas over a
// chunk of rows and streams every layer's source rows through a small LDS ring per plane — 8 luma rows and 4 chroma rows of 128
// bytes, 1.5 KB per layer — filled four (two) rows at a time by `global_load_lds_dwordx4`: a lane's 16 bytes go straight from its own
// global address to LDS at M0 + lane * 16 (tools/probe_lds_dma.cpp), no registers, no LDS write instruction.  With every layer's
// rows resident the loop runs over canvas rows: row entry, weights, tap addresses once, then per layer 12 taps, the integer
// matrix and one blend on float codes, one pack and one store at the end.  Same operations per pixel and layer as
// apply_layer_bgra / tick_bgra_wave (the blend result of a layer is rounded to codes exactly as its store would round it), so the
// same bytes.
//
// Eligibility is decided on the host (tick_route.cpp: bgra_stream_eligible): cleared BGRA canvas, every tick the same number (<= 4) of NV12
// layers, layers 1.. flagged LF_SAME_GEOM, axis-aligned bounded matrices without flips, no fill paint, opacities in [0, 1],
// horizontal reduction <= 1.7 (a strip's source bytes fit the ring's 128-byte rows), plane rows a multiple of 16 bytes.
#include "kernels_stream_body.hip.inc"
#include "stream_select.h"

namespace chv {

// the phased plan's shape (stream_plan.h: StreamPlanShape; profiles/stream_plan_notes.md has the candidates' numbers)
#ifndef CHV_STREAM_PLAN_TALL
#define CHV_STREAM_PLAN_TALL 240
#endif
#ifndef CHV_STREAM_PLAN_CLOSING_DEN
#define CHV_STREAM_PLAN_CLOSING_DEN 4
#endif
#ifndef CHV_STREAM_PLAN_TALL_TENTHS
#define CHV_STREAM_PLAN_TALL_TENTHS 10      // the gate: the tall phase alone holds at least one round of the chip's wave slots (20 and 5 measured beside it)
#endif
#ifndef CHV_STREAM_PLAN_SHORTEST
#define CHV_STREAM_PLAN_SHORTEST 24
#endif

// kernels_stream_opq.hip.cpp: the opaque-bottom kernels (2 - 4 layers, absorbed matrices), same grid, LDS and arguments
hipError_t launch_bgra_stream_opaque(const DTick *ticks_host, const DLayer *layers_host, const DTick *ticks, const DLayer *layers, int n_ticks, bool planar, dim3 grid,
                                     size_t lds, int strips_x, const StreamPlan &plan, hipStream_t stream);

template <int NL, bool PL, bool ABS>
__global__ __launch_bounds__(64 * ST_WAVES, CHV_STREAM_WAVES) void tick_bgra_stream(const DTick *__restrict__ ticks, const DLayer *__restrict__ layers, int strips_x,
                                                                          const StreamPlan plan) {
    stream_body<NL, false, PL, ABS>(ticks, layers, strips_x, plan);
}

template <int NL, bool PL, bool ABS>
__global__ __launch_bounds__(64 * ST_WAVES, CHV_STREAM_WAVES) void tick_bgra_stream_one(const StreamOne<NL> a, int strips_x, int chunks_y, int rows_per_chunk) {
    stream_body<NL, true, PL, ABS>(&a.t, a.l, strips_x, StreamUniform{ chunks_y, rows_per_chunk });
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// (which launches take these kernels — bgra_stream_eligible —: tick_route.cpp)
#define CHV_STR2(x) #x
#define CHV_STR(x) CHV_STR2(x)
// what this translation unit was built with (chv_build_flags; a timing-only CHV_ST_ABL build must never ship)
const char *bgra_stream_build_flags() { return "tick_bgra_stream:abl=" CHV_STR(CHV_ST_ABL) ",strips_per_block=" CHV_STR(CHV_STREAM_BLOCK) ",rounds=" CHV_STR(CHV_STREAM_ROUNDS); }

// ticks == nullptr: one tick, launched with its descriptors (ticks_host[0], layers_host) as kernel arguments
hipError_t launch_bgra_stream(const DTick *ticks_host, const DLayer *layers_host, const DTick *ticks, const DLayer *layers, int n_ticks, int maxW, int maxH, hipStream_t stream) {
    const int nl = ticks_host[0].n_layers;
    const int strips_x = (maxW + 63) / 64;
    // rows per chunk.  The uniform rule (stream_plan.h: stream_uniform_rows).  Launches that fill the chip: tall chunks amortise the per-chunk
    // geometry and the first ring fill — enough chunks for CHV_STREAM_ROUNDS rounds of waves.  Small launches (a Swift VideoMixer issues ONE tick and
    // waits): a wave's rows are a serial chain — a lone wave issues an instruction every ~2.3 ns and sits out every memory round trip itself — so
    // the chain is cut short, down to 4 rows, until about 4 800 waves share the launch (tools/stream_rows_sweep.sh, 720p ticks, us per launch at
    // 4 / 6 / 8 / 12 / 16 / 24 rows: one tick 10.9 / 12.4 / 13.2 / 18.0 / 20.0 / 28.2; two 18.9 / 17.6 / 18.8 / 21.9 / 24.0 / 33.7; eight 54.2 / 51.2 /
    // 51.8 / 51.0 / 54.6 / 52.3; sixteen 104.5 / 97.2 / 95.7 / 91.6 / 93.8 / 94.3).
    // Batches whose tall phase alone fills the chip once are PHASED (stream_plan.h: tall chunks first, short ones at the end; CHV_STREAM_PLAN,
    // profiles/stream_plan_notes.md); a forced or fixed height, the by-value lone tick and everything smaller keep one uniform phase.
    StreamRowsRule rule;
    rule.want_waves = 1024L * CHV_STREAM_WAVES * CHV_STREAM_ROUNDS;
    rule.small_waves = CHV_STREAM_SMALL_WAVES;
    rule.small_rows_max = CHV_STREAM_SMALL_ROWS_MAX;
    rule.min_rows = CHV_STREAM_MIN_ROWS;
    rule.rows_fixed = CHV_STREAM_ROWS_FIXED;                                              // (sweeps: tools/build_variant.sh ... -DCHV_STREAM_ROWS_FIXED=n)
    rule.rows_forced = switches().stream_rows.load(std::memory_order_relaxed);            // (tests: CHV_STREAM_ROWS)
    // CHV_STREAM_PLAN: 0 uniform only; 1 the planner decides for this chip — the tall phase alone must hold CHV_STREAM_PLAN_TALL_TENTHS / 10 rounds of
    // the launched kernels' wave slots (the chroma-carry kernels run five waves per SIMD); N >= 2 (tests) as if the chip held N waves and a
    // tenth of a round were enough, so that batches of a few small ticks are phased and N decides at which tall height
    const int plan_switch = switches().stream_plan.load(std::memory_order_relaxed);
    StreamPlanShape shape;
    shape.tall = plan_switch ? CHV_STREAM_PLAN_TALL : 0;
    shape.closing_den = CHV_STREAM_PLAN_CLOSING_DEN;
    shape.shortest = CHV_STREAM_PLAN_SHORTEST;
    shape.tall_tenths = plan_switch >= 2 ? 1 : CHV_STREAM_PLAN_TALL_TENTHS;
    const bool planar = layers_host[ticks_host[0].first_layer].kind == LK_BGRA_FROM_Y420P;
    // the absorbed form of the colour matrix (pixel_math.hip.h) when every layer's matrix has one — all but BT.601 full range
    bool absorb = CHV_STREAM_ABSORB != 0;
    for (int i = 0; i < n_ticks && absorb; i++)
        for (int l = 0; l < nl; l++) absorb = absorb && csc_absorbable(layers_host[ticks_host[i].first_layer + l].csc);
    // the opaque-bottom kernels when every tick's bottom layer has opacity exactly 1 (a mixer's base feed: stream_select.h).  Plain-matrix
    // launches (BT.601 full range) keep the general kernels: the opaque-bottom form exists for the absorbed matrix only.
    const bool opaque = absorb && stream_opaque_bottom(ticks_host, layers_host, n_ticks, switches().stream_opaque.load(std::memory_order_relaxed));
    // (what launch_bgra_stream_opaque will ask: the chroma-carry kernels and their f32-tap form run five waves per SIMD)
    const bool five_waves = opaque && stream_chroma_carry(ticks_host, layers_host, n_ticks, planar, !ticks, switches().stream_carry.load(std::memory_order_relaxed));
    const long slots = plan_switch >= 2 ? plan_switch : 1024L * (five_waves ? 5 : CHV_STREAM_WAVES);
    const StreamPlan plan = stream_plan_make(n_ticks, strips_x, maxH, slots, !ticks, rule, shape, ST_WAVES);
    const int chunks_y = plan.ph[0].chunks_y, rows = plan.ph[0].rows;                     // (the by-value lone tick: always one phase)
    const bool phased = stream_plan_phases(plan) > 1;
    dim3 grid((unsigned)stream_plan_blocks(plan, strips_x, ST_WAVES));
    const size_t layer_bytes = planar ? (size_t)st_layer_bytes<1, true>() : (size_t)st_layer_bytes<1, false>();
    size_t lds = (size_t)ST_WAVES * ((size_t)nl * layer_bytes + ST_TAB * (sizeof(uint4) + sizeof(uint32_t)));
    if (CHV_STREAM_LDS_MIN > 0) lds = std::max<size_t>(lds, CHV_STREAM_LDS_MIN);      // (occupancy A/Bs: tools/build_variant.sh ... -DCHV_STREAM_LDS_MIN=n)
    if (opaque) {
        const hipError_t err = launch_bgra_stream_opaque(ticks_host, layers_host, ticks, layers, n_ticks, planar, grid, lds, strips_x, plan, stream);
        if (err == hipSuccess) debug_counters().stream_opaque_launches.fetch_add(1, std::memory_order_relaxed);
        if (err == hipSuccess && phased) debug_counters().stream_phased_launches.fetch_add(1, std::memory_order_relaxed);
        return err;
    }
    if (!ticks) {
        // one tick, descriptors as kernel arguments (launch_transient)
        if (n_ticks != 1 || !layers_host) return hipErrorInvalidValue;
        auto go = [&](auto tag) {
            constexpr int NL = decltype(tag)::value;
            StreamOne<NL> a;
            a.t = ticks_host[0];
            a.t.first_layer = 0;
            for (int l = 0; l < NL; l++) a.l[l] = layers_host[ticks_host[0].first_layer + l];
            auto fire = [&](auto pl, auto ab) {
                hipLaunchKernelGGL((tick_bgra_stream_one<NL, decltype(pl)::value, decltype(ab)::value>), grid, dim3(64 * ST_WAVES), lds, stream, a, strips_x, chunks_y, rows);
            };
            if (planar) { if (absorb) fire(std::true_type{}, std::true_type{}); else fire(std::true_type{}, std::false_type{}); }
            else { if (absorb) fire(std::false_type{}, std::true_type{}); else fire(std::false_type{}, std::false_type{}); }
        };
        switch (nl) {
        case 1: go(std::integral_constant<int, 1>{}); break;
        case 2: go(std::integral_constant<int, 2>{}); break;
        case 3: go(std::integral_constant<int, 3>{}); break;
        default: go(std::integral_constant<int, 4>{}); break;
        }
        return hipGetLastError();
    }
#define CHV_ST_GO2(N, P, A) hipLaunchKernelGGL((tick_bgra_stream<N, P, A>), grid, dim3(64 * ST_WAVES), lds, stream, ticks, layers, strips_x, plan)
#define CHV_ST_GO(N) do { if (planar) { if (absorb) CHV_ST_GO2(N, true, true); else CHV_ST_GO2(N, true, false); } \
                          else { if (absorb) CHV_ST_GO2(N, false, true); else CHV_ST_GO2(N, false, false); } } while (0)
    switch (nl) {
    case 1: CHV_ST_GO(1); break;
    case 2: CHV_ST_GO(2); break;
    case 3: CHV_ST_GO(3); break;
    default: CHV_ST_GO(4); break;
    }
#undef CHV_ST_GO
#undef CHV_ST_GO2
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess && phased) debug_counters().stream_phased_launches.fetch_add(1, std::memory_order_relaxed);
    return err;
}

}  // namespace chv
