// kernels_stream_carry.hip.cpp — tick_bgra_stream_cc: the opaque-bottom kernels of tick_bgra_stream (kernels_stream_opq.hip.cpp) with the chroma
// taps CARRIED down the lane from one canvas row to the next (stream_body: CRY, kernels_stream_body.hip.inc).  Where the chroma plane advances
// by at most one row per canvas row — every enlargement, and reductions up to 2 : 1, the headline's 1.5 : 1 among them — a row reads the
// chroma bytes of the ring rows that are new to the lane (4 per layer on three rows in four at 1.5 : 1, none on the fourth) instead of all 8:
// about 30 LDS instructions per four-layer row where the transient form issues 50.  The carried bytes are 8 registers per layer, live across
// rows: these kernels take up to 96 VGPRs, five waves per SIMD where their siblings run six.  Same bytes as the kernels they replace:
// launch_bgra_stream_opaque picks these for batch launches of NV12 sources when stream_select.h says so, CHV_STREAM_CARRY=0 keeps the others.
#include "kernels_stream_body.hip.inc"

namespace chv {

#ifndef CHV_STREAM_CARRY_WAVES
#define CHV_STREAM_CARRY_WAVES 5
#endif

template <int NL>
__global__ __launch_bounds__(64 * ST_WAVES, CHV_STREAM_CARRY_WAVES) void tick_bgra_stream_cc(const DTick *__restrict__ ticks, const DLayer *__restrict__ layers, int strips_x,
                                                                                   const StreamPlan plan) {
    stream_body<NL, false, false, true, true, true>(ticks, layers, strips_x, plan);
}

// a batch launch (descriptors on the device) of `nl` = 2 .. 4 NV12 layers with absorbed matrices and opaque bottoms; grid, LDS and arguments
// are those of the kernels it replaces
hipError_t launch_bgra_stream_carry(int nl, const DTick *ticks, const DLayer *layers, int n_ticks, dim3 grid, size_t lds, int strips_x, const StreamPlan &plan,
                                    hipStream_t stream) {
    if (!ticks || !layers) return hipErrorInvalidValue;
    switch (nl) {
    case 2: hipLaunchKernelGGL((tick_bgra_stream_cc<2>), grid, dim3(64 * ST_WAVES), lds, stream, ticks, layers, strips_x, plan); break;
    case 3: hipLaunchKernelGGL((tick_bgra_stream_cc<3>), grid, dim3(64 * ST_WAVES), lds, stream, ticks, layers, strips_x, plan); break;
    case 4: hipLaunchKernelGGL((tick_bgra_stream_cc<4>), grid, dim3(64 * ST_WAVES), lds, stream, ticks, layers, strips_x, plan); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace chv
