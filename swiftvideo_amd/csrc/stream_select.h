// stream_select.h — which form of tick_bgra_stream a launch takes (host side only; launch_bgra_stream, kernels_stream.hip.cpp).
#pragma once
#include "device_types.h"

#include <string.h>

namespace chv {

// The opaque-bottom kernels (kernels_stream_opq.hip.cpp) compute no blend for layer 0: they are right only where its opacity is EXACTLY 1
// — bit-equal, 0.99999994f is not — in every tick of the launch, and there is a layer 1 to take its code.  `enabled`: CHV_STREAM_OPAQUE.
inline bool stream_opaque_bottom(const DTick *ticks_host, const DLayer *layers_host, int n_ticks, int enabled) {
    if (!enabled || n_ticks < 1) return false;
    const float one = 1.0f;
    for (int i = 0; i < n_ticks; i++) {
        if (ticks_host[i].n_layers < 2) return false;
        if (memcmp(&layers_host[ticks_host[i].first_layer].u[U_OPACITY], &one, sizeof one) != 0) return false;
    }
    return true;
}

// The chroma-carry kernels (kernels_stream_carry.hip.cpp) keep a lane's chroma taps from one canvas row to the next and read only the ring
// rows that are new to it: right for every geometry the opaque-bottom kernels take, but a gain only where the chroma plane advances by AT MOST
// ONE row per canvas row (two new rows per canvas row are the eight reads of the transient form, paid at five waves per SIMD instead of
// six).  Chroma rows per canvas row, as bgra_stream_eligible bounds the luma ratio: v = (y / H * 2 - 1) * T5 * X5 + ..., so dv/dy * h = 2 T5 X5 h / H
// with the chroma plane's h.  Layers 1.. of a tick share layer 0's geometry (LF_SAME_GEOM).  Only launches the opaque-bottom branch takes are
// asked; they exist for NV12 batches — planar sources and the by-value lone tick keep tick_bgra_stream_ob.  `enabled`: CHV_STREAM_CARRY.
inline bool stream_chroma_carry(const DTick *ticks_host, const DLayer *layers_host, int n_ticks, bool planar, bool by_value, int enabled) {
    if (!enabled || planar || by_value || n_ticks < 1) return false;
    for (int i = 0; i < n_ticks; i++) {
        const DTick &T = ticks_host[i];
        if (T.n_layers < 2 || T.n_layers > 4 || T.H < 1) return false;
        const DLayer &Y = layers_host[T.first_layer];
        const double ky = 2.0 * (double)Y.u[U_TRANSFORM + 5] * (double)Y.u[U_TEXTURE + 5];
        const double sc = ky * Y.src.pl[1].h / (double)T.H;
        if (!(sc > 0.0) || !(sc <= 1.0)) return false;
    }
    return true;
}

}  // namespace chv
