// lanczos_to_420_body.hip.h — the row code of the planar Lanczos-3 resampler for the source packings lanczos_420_body.hip.h cannot express
// (DESIGN.md section 4.4.9), for kernels_lanczos_to_420.hip.cpp (chv_scale_lanczos_to_420, chv_scale_lanczos_to_420_ladder).  The arithmetic
// is that of lanczos_planar_body.hip.h, logical image by logical image, so the bytes are.  Luma and planar chroma ARE planar_strip<T, 1>,
// two planar chroma planes into a CbCr plane ARE x420_strip<T, true>, one component of a 2-component plane into a 1-component plane (NV21's
// chroma into y420p, the Y of yuvs / zvuy) IS x420_strip<T, false>.  What is here is chroma read from ONE interleaved plane at a byte offset
// per target component — strip_core (lanczos_strip_core.hip.h) under one more column description:
//
//   to420_strip<T, 2, 2>   NV21 -> NV12.  The target is the CbCr plane; even lanes (Cb) read byte 1 of the source's texels, odd lanes (Cr) byte 0.
//   to420_strip<T, 4, 1>   yuvs / zvuy -> one chroma plane of y420p.  A chroma texel is four bytes of the packed row (two pixels); the taps are
//                          four bytes apart from byte `off0` (yuvs: Cb 1, Cr 3; zvuy: Cb 0, Cr 2).  One dword per tap, no realignment; a
//                          lane outside the row replicates the whole dword (its Y bytes ride along; no chroma lane reads them).
//   to420_strip<T, 4, 2>   yuvs / zvuy -> NV12's CbCr plane.  Even lanes start at `off0` (Cb), odd lanes at `off1` (Cr).
//
// The tile route needs nothing new: x420_tile takes a start pointer per component and a tap stride.
#pragma once
#include "lanczos_420_body.hip.h"

#pragma clang fp contract(off)

namespace chv {

// One strip of one chroma target plane of OC components, fed from one plane whose texels are SC bytes: g.src has the LOGICAL image's size
// (texels of SC bytes), the plane's start and pitch.
template <int T, int SC, int OC>
CHV_DEV void to420_strip(const PlanarPlane &g, int off0, int off1, int strip, int chunk, int rows_per_wave, uint8_t *lsm) {
    static_assert(SC == 2 || SC == 4, "an interleaved source");
    strip_core<T, StripCols<SC, OC>>(g, g.src, off0, off1, strip, chunk, rows_per_wave, lsm, OpenByteQuads{});
}

}  // namespace chv
