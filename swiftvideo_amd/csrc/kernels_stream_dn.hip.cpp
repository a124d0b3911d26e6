// kernels_stream_dn.hip.cpp — tick_bgra_stream_cd: the chroma-carry kernels of tick_bgra_stream (kernels_stream_carry.hip.cpp) with their taps on
// the full-rate f32 multiplier (stream_body: DN, kernels_stream_body.hip.inc; cs_mix_d, pixel_math.hip.h).  The byte a tap read leaves in its
// register is the binary32 denormal b x 2^-149: with 2^127 on the column weights the twelve taps of a layer are v_fma_f32 / v_fmac_f32 where
// the sibling issues v_fma_mix_f32, and the 2^-22 they carry leaves on the add that converts the sample.  Same bytes, same rings, reads and
// waits as the sibling: launch_bgra_stream_opaque picks these for every launch the carry kernels take while CHV_STREAM_F32TAPS is on (default;
// profiles/f32_denormal_taps_notes.md).
#include "kernels_stream_body.hip.inc"

namespace chv {

template <int NL>
__global__ __launch_bounds__(64 * ST_WAVES, 5) void tick_bgra_stream_cd(const DTick *__restrict__ ticks, const DLayer *__restrict__ layers, int strips_x,
                                                                      const StreamPlan plan) {
    stream_body<NL, false, false, true, true, true, /*DN*/ true>(ticks, layers, strips_x, plan);
}

// grid, LDS and arguments are those of the chroma-carry kernels
hipError_t launch_bgra_stream_f32taps(int nl, const DTick *ticks, const DLayer *layers, int n_ticks, dim3 grid, size_t lds, int strips_x, const StreamPlan &plan,
                                      hipStream_t stream) {
    if (!ticks || !layers) return hipErrorInvalidValue;
    switch (nl) {
    case 2: hipLaunchKernelGGL((tick_bgra_stream_cd<2>), grid, dim3(64 * ST_WAVES), lds, stream, ticks, layers, strips_x, plan); break;
    case 3: hipLaunchKernelGGL((tick_bgra_stream_cd<3>), grid, dim3(64 * ST_WAVES), lds, stream, ticks, layers, strips_x, plan); break;
    case 4: hipLaunchKernelGGL((tick_bgra_stream_cd<4>), grid, dim3(64 * ST_WAVES), lds, stream, ticks, layers, strips_x, plan); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace chv
