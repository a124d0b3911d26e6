// lanczos_ladder_launch.hip.h — the launches of one chunk of a Lanczos ladder, for every ladder unit: the rungs of the strip route in one
// launch, the rungs of the tile route in at most one more (lanczos_ladder_grid.h: how their grids are numbered).
#pragma once
#include <hip/hip_runtime.h>

#include "lanczos_ladder_grid.h"

namespace chv {

// launch_strip / launch_tile: one hipLaunchKernelGGL each.  *launches counts the launches made, also when the second of two fails.
template <class Strip, class Tile>
inline hipError_t ladder_launch(int *launches, bool strip, Strip launch_strip, bool tile, Tile launch_tile) {
    (void)hipGetLastError();
    if (strip) {
        launch_strip();
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
    }
    if (tile) {
        launch_tile();
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
    }
    return hipSuccess;
}

}  // namespace chv
