// kernels_stream_opq.hip.cpp — tick_bgra_stream_ob: tick_bgra_stream (kernels_stream.hip.cpp, kernels_stream_body.hip.inc) for ticks whose bottom
// layer is opaque — a mixer's base feed under its overlays, the bench headline's tick.  On the cleared canvas such a layer's blend is its
// own code: the row computes none for it, and layer 1 takes the code times its 1 - opacity in one v_fma_mix_f32 per channel (stream_body: OPQ;
// six vector instructions fewer per row).  Same bytes as the kernels it replaces: launch_bgra_stream picks these for 2 - 4 layers of
// absorbed colour matrices when stream_select.h says so, CHV_STREAM_OPAQUE=0 keeps the others.  NV12 batches whose chroma advances by at
// most a row per canvas row go on to tick_bgra_stream_cc (kernels_stream_carry.hip.cpp) from here.
#include "kernels_stream_body.hip.inc"
#include "stream_select.h"

namespace chv {

// kernels_stream_carry.hip.cpp: the chroma-carry kernels (NV12 batches of 2 - 4 layers), same grid, LDS and arguments
hipError_t launch_bgra_stream_carry(int nl, const DTick *ticks, const DLayer *layers, int n_ticks, dim3 grid, size_t lds, int strips_x, const StreamPlan &plan,
                                    hipStream_t stream);
// kernels_stream_dn.hip.cpp: the same kernels with their taps on the f32 multiplier (CHV_STREAM_F32TAPS)
hipError_t launch_bgra_stream_f32taps(int nl, const DTick *ticks, const DLayer *layers, int n_ticks, dim3 grid, size_t lds, int strips_x, const StreamPlan &plan,
                                      hipStream_t stream);

template <int NL, bool PL, bool ABS>
__global__ __launch_bounds__(64 * ST_WAVES, CHV_STREAM_WAVES) void tick_bgra_stream_ob(const DTick *__restrict__ ticks, const DLayer *__restrict__ layers, int strips_x,
                                                                             const StreamPlan plan) {
    stream_body<NL, false, PL, ABS, true>(ticks, layers, strips_x, plan);
}

template <int NL, bool PL, bool ABS>
__global__ __launch_bounds__(64 * ST_WAVES, CHV_STREAM_WAVES) void tick_bgra_stream_ob_one(const StreamOne<NL> a, int strips_x, int chunks_y, int rows_per_chunk) {
    stream_body<NL, true, PL, ABS, true>(&a.t, a.l, strips_x, StreamUniform{ chunks_y, rows_per_chunk });
}

// ticks == nullptr: one tick, launched with its descriptors as kernel arguments (launch_bgra_stream)
hipError_t launch_bgra_stream_opaque(const DTick *ticks_host, const DLayer *layers_host, const DTick *ticks, const DLayer *layers, int n_ticks, bool planar, dim3 grid,
                                     size_t lds, int strips_x, const StreamPlan &plan, hipStream_t stream) {
    const int nl = ticks_host[0].n_layers;
    if (nl < 2 || nl > 4) return hipErrorInvalidValue;
    // NV12 batches whose chroma advances by at most one row per canvas row: the chroma taps carried from row to row (stream_select.h)
    if (stream_chroma_carry(ticks_host, layers_host, n_ticks, planar, !ticks, switches().stream_carry.load(std::memory_order_relaxed))) {
        const bool f32taps = switches().stream_f32taps.load(std::memory_order_relaxed) != 0;
        const hipError_t err = f32taps ? launch_bgra_stream_f32taps(nl, ticks, layers, n_ticks, grid, lds, strips_x, plan, stream)
                                       : launch_bgra_stream_carry(nl, ticks, layers, n_ticks, grid, lds, strips_x, plan, stream);
        if (err == hipSuccess) debug_counters().stream_carry_launches.fetch_add(1, std::memory_order_relaxed);
        if (err == hipSuccess && f32taps) debug_counters().stream_f32tap_launches.fetch_add(1, std::memory_order_relaxed);
        return err;
    }
    auto go = [&](auto tag, auto pl) {
        constexpr int NL = decltype(tag)::value;
        constexpr bool PL = decltype(pl)::value;
        if (!ticks) {
            StreamOne<NL> a;
            a.t = ticks_host[0];
            a.t.first_layer = 0;
            for (int l = 0; l < NL; l++) a.l[l] = layers_host[ticks_host[0].first_layer + l];
            hipLaunchKernelGGL((tick_bgra_stream_ob_one<NL, PL, true>), grid, dim3(64 * ST_WAVES), lds, stream, a, strips_x, plan.ph[0].chunks_y, plan.ph[0].rows);
        } else {
            hipLaunchKernelGGL((tick_bgra_stream_ob<NL, PL, true>), grid, dim3(64 * ST_WAVES), lds, stream, ticks, layers, strips_x, plan);
        }
    };
    auto layers_of = [&](auto pl) {
        switch (nl) {
        case 2: go(std::integral_constant<int, 2>{}, pl); break;
        case 3: go(std::integral_constant<int, 3>{}, pl); break;
        default: go(std::integral_constant<int, 4>{}, pl); break;
        }
    };
    if (!ticks && (n_ticks != 1 || !layers_host)) return hipErrorInvalidValue;
    if (planar) layers_of(std::true_type{}); else layers_of(std::false_type{});
    return hipGetLastError();
}

}  // namespace chv
