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

}  // namespace chv
