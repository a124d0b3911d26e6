// tests/stubhip/stub_lanczos_planar_launcher.cpp — the stand-in for kernels_lanczos_planar.hip.cpp in the sanitizer builds
// (tests/test_lanczos_planar_sanitizers.py).  TEST INFRASTRUCTURE.  The "kernel" is a closure on the stream that, when the stream gets to it,
// reads the first and last entry of every table and touches the first and last byte of every plane — a batch's plane pairs are read LATE, from
// the descriptor slot: a table freed while a launch still needs it, a slot overwritten too early, a source freed under a queued launch or a
// plane whose extent was not checked is a sanitizer report.  Every target plane's first byte counts the launches that wrote it.
#include <hip/hip_runtime.h>

#include "../../swiftvideo_amd/csrc/lanczos_planar.h"

namespace chv {
static unsigned touch_plane(const DPlane &d, const DPlane &s) {
    const volatile uint8_t *sp = s.ptr;
    const unsigned sum = sp[0] + sp[(size_t)(s.h - 1) * s.pitch + (size_t)s.w * s.comps - 1];
    volatile uint8_t *dp = d.ptr;
    const size_t last = (size_t)(d.h - 1) * d.pitch + (size_t)d.w * d.comps - 1;
    dp[0] = (uint8_t)(dp[0] + 1);
    if (last) dp[last] = (uint8_t)(0xA5 ^ (sum & 1));
    return sum;
}
static hipError_t stub_lanczos_planar(const LanczosPlanarJob &job_in, hipStream_t stream) {
    if (stubhip_launch_should_fail()) return hipErrorLaunchFailure;
    if (job_in.n_planes < 2 || job_in.n_planes > kLanczosPlanarMaxPlanes || job_in.n_pictures < 1) return hipErrorInvalidValue;
    const LanczosPlanarJob job = job_in;
    stubhip_enqueue(stream, [job] {
        volatile float sink = 0.f;
        for (int p = 0; p < job.n_planes; p++) {
            const LanczosPlaneTables &t = job.tab[p];
            const int ow = job.dst[p].w, oh = job.dst[p].h;
            sink = sink + (float)t.fx[0] + (float)t.fx[ow - 1] + t.wx[0] + t.wx[(size_t)ow * t.tx - 1];
            sink = sink + (float)t.fy[0] + (float)t.fy[oh - 1] + t.wy[0] + t.wy[(size_t)oh * t.ty - 1];
        }
        for (int i = 0; i < job.n_pictures; i++)
            for (int p = 0; p < job.n_planes; p++) {
                const DPlane d = job.batch ? job.batch[((size_t)i * job.n_planes + p) * 2] : job.dst[p];
                const DPlane s = job.batch ? job.batch[((size_t)i * job.n_planes + p) * 2 + 1] : job.src[p];
                (void)touch_plane(d, s);
            }
    });
    return hipSuccess;
}
static const struct Registrar { Registrar() { register_lanczos_planar_launcher(stub_lanczos_planar); } } g_registrar;
}  // namespace chv
