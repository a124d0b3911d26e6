// tests/stubhip/stub_lanczos_refuses.h — the 160 KB rule of chv_scale_lanczos as the stub launchers of the Lanczos units ask it, one image's
// own sizes at a time.  TEST INFRASTRUCTURE: an independent restatement of the formula, on purpose not the product's header
// (swiftvideo_amd/csrc/lanczos_route.h) — the stress programs compare what the product's host path refuses with what this says.
#pragma once
#include <stddef.h>

namespace chv {

static inline bool stub_lanczos_refuses(int dw, int dh, int sw, int sh, int tx, int ty) {
    const double sy = (double)sh / (double)dh, sx = (double)sw / (double)dw;
    const int max_rows = (int)(3 * sy + 2) + ty;
    const int max_cols = ((int)(7 * sx + 2) + tx + 3) & ~3;
    return (size_t)max_rows * 8 * 16 + (size_t)max_rows * max_cols * 4 > 160 * 1024;
}

}  // namespace chv
