// lanczos_planar.h — what chv_scale_lanczos (chipvideo.cpp) and the planar Lanczos unit (kernels_lanczos_planar.hip.cpp) share.
//
// A 4:2:0 picture (NV12: planes of 1 and 2 components, y420p: three planes of 1) is resampled plane by plane, every plane with the
// tables of its OWN width and height — and all planes of a picture, and all pictures of a batch chunk, in ONE launch.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"

namespace chv {

// The tables of one plane pair.  `fx` / `fy`: first source texel / row of every output column / row (may lie outside the plane: the kernels
// clamp the load address); `wx` / `wy`: tx / ty weights per output column / row.  Device memory that stays valid until the launch has run.
struct LanczosPlaneTables {
    const int32_t *fx; const float *wx;
    const int32_t *fy; const float *wy;
    int32_t tx, ty;
};

constexpr int kLanczosPlanarMaxPlanes = 3;

struct LanczosPlanarJob {
    int32_t n_planes;                                  // 2 (NV12) or 3 (y420p)
    LanczosPlaneTables tab[kLanczosPlanarMaxPlanes];
    // picture 0's planes — (dst, src) per plane; every picture of a batch has these sizes and component counts
    DPlane dst[kLanczosPlanarMaxPlanes], src[kLanczosPlanarMaxPlanes];
    // batch != nullptr: n_pictures pictures, picture i's plane p at batch[(i * n_planes + p) * 2] (target) and + 1 (source), in memory the
    // device can read that stays unchanged until the launch has run.  nullptr: the one picture above travels in the launch's arguments.
    const DPlane *batch;
    int32_t n_pictures;
};

// One launch.  Reports like every launcher, through its return value; hipErrorInvalidValue for a refused plane (nothing is launched).
typedef hipError_t (*LanczosPlanarLauncher)(const LanczosPlanarJob &job, hipStream_t stream);

// chipvideo.cpp owns the pointer (null: no kernel unit in this build — the YUV families answer CHV_ERR_NOT_IMPLEMENTED); the kernel unit
// registers its launcher when the library is loaded.  The host units therefore link without it (tests/stubhip).
void register_lanczos_planar_launcher(LanczosPlanarLauncher fn);

}  // namespace chv
