// lanczos_strip_parts.hip.h — what every wave-per-strip Lanczos-3 body is built from: lanczos3_strip<T>
// (kernels_lanczos.hip.cpp), lanczos_yuv_strip_body (lanczos_to_yuv_body.hip.h), rgb_strip<T> (lanczos_rgb_body.hip.h) and strip_core
// (lanczos_strip_core.hip.h, the body of planar_strip, x420_strip, to420_strip, hbd_strip and fy_strip).  The bodies differ in their windows and in
// where a finished row goes; these pieces they spell alike.
#pragma once
#include "pixel_math.hip.h"

#include <cstddef>
#include <type_traits>
#include <utility>

namespace chv {

// f(0) && f(1) && ... && f(N - 1) with the index a compile-time constant in every call: how a strip body walks the T source rows of a trip.
// A fold expression, not `#pragma unroll`: with the early exit and the inner loop the unroller gives up from 10 taps on, and a window
// indexed at run time lives in scratch memory.
template <typename F, int... Is>
CHV_DEV bool lanczos_all_of(F &&f, std::integer_sequence<int, Is...>) { return (... && f(std::integral_constant<int, Is>{})); }

// hand-awaited prefetch depth of a body whose trip is T source rows: a divisor of T, so that a row's slot is static in every copy of the body
template <int T> struct LanczosPre { static constexpr int value = T % 4 == 0 ? 4 : T % 3 == 0 ? 3 : 2; };

// LDS in front of the staging ring: the vertical weights of a wave's output rows, T per row
constexpr size_t lanczos_wtab_bytes(int rows, int T) { return ((size_t)rows * T * sizeof(float) + 15) & ~(size_t)15; }

// The vertical weights of a strip's output rows [j0, j0 + nrows), zero-padded IN FRONT to the window's T rows (ty <= T), go to LDS before the
// row loop (after it every wait for a global load would also wait for the row prefetch: one counter); the vertical chain reads a row of them
// at one address for all lanes.  (Through the scalar unit instead, 22 loads at computed offsets per output row: <22> spills SGPRs.)
template <int T>
CHV_DEV void lanczos_fill_wtab(float *wtab, const float *__restrict__ wy, int ty, int j0, int nrows, int lane) {      // wtab: [nrows][T]
    const int pad = T - ty;                                        // window rows in front of a vertical filter's first tap
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
}

}  // namespace chv
