// tests/stubhip/stub_lanczos_to_yuv_launcher.cpp — the stand-in for kernels_lanczos_to_yuv.hip.cpp in the sanitizer builds
// (tests/test_lanczos_to_yuv_sanitizers.py).  TEST INFRASTRUCTURE.  The "kernel" is a closure on the stream that, when the stream gets to it,
// reads the first and last entry of both tables and touches the first and last byte of every plane — a batch's planes are read LATE, from the
// descriptor slot: a table freed while a launch still needs it, a slot overwritten too early, a source freed under a queued launch or a plane
// whose extent was not checked is a sanitizer report.  Every target plane's first byte counts the launches that wrote it.
#include <hip/hip_runtime.h>

#include "../../swiftvideo_amd/csrc/lanczos_to_yuv.h"

namespace chv {
static hipError_t stub_lanczos_to_yuv(const LanczosToYuvJob &job_in, hipStream_t stream) {
    if (stubhip_launch_should_fail()) return hipErrorLaunchFailure;
    if ((job_in.n_dst != 2 && job_in.n_dst != 3) || job_in.n_pictures < 1) return hipErrorInvalidValue;
    // (the matrix arrives in the source's byte order: rows that sum to the luma gain and to zero whatever the order is)
    if (job_in.ku[0] + job_in.ku[1] + job_in.ku[2] != 0 || job_in.kv[0] + job_in.kv[1] + job_in.kv[2] != 0 || job_in.ky[1] < job_in.ky[0]) return hipErrorInvalidValue;
    const LanczosToYuvJob job = job_in;
    stubhip_enqueue(stream, [job] {
        volatile float sink = 0.f;
        const int ow = job.dst[0].w, oh = job.dst[0].h;
        sink = sink + (float)job.fx[0] + (float)job.fx[ow - 1] + job.wx[0] + job.wx[(size_t)ow * job.tx - 1];
        sink = sink + (float)job.fy[0] + (float)job.fy[oh - 1] + job.wy[0] + job.wy[(size_t)oh * job.ty - 1];
        for (int i = 0; i < job.n_pictures; i++) {
            const DPlane s = job.batch ? job.batch[(size_t)i * (job.n_dst + 1) + job.n_dst] : job.src;
            const volatile uint8_t *sp = s.ptr;
            const unsigned sum = sp[0] + sp[(size_t)(s.h - 1) * s.pitch + (size_t)s.w * s.comps - 1];
            for (int p = 0; p < job.n_dst; p++) {
                const DPlane d = job.batch ? job.batch[(size_t)i * (job.n_dst + 1) + p] : job.dst[p];
                volatile uint8_t *dp = d.ptr;
                const size_t last = (size_t)(d.h - 1) * d.pitch + (size_t)d.w * d.comps - 1;
                dp[0] = (uint8_t)(dp[0] + 1);
                if (last) dp[last] = (uint8_t)(0xA5 ^ (sum & 1));
            }
        }
    });
    return hipSuccess;
}
static const struct ToYuvRegistrar { ToYuvRegistrar() { register_lanczos_to_yuv_launcher(stub_lanczos_to_yuv); } } g_to_yuv_registrar;
}  // namespace chv
