// tests/stubhip/stub_lanczos_from_yuv_launcher.cpp — the stand-in for kernels_lanczos_from_yuv.hip.cpp in the sanitizer builds
// (tests/test_lanczos_from_yuv_sanitizers.py).  TEST INFRASTRUCTURE.  Like the unit it stands for, it checks both logical planes before
// anything is enqueued (the 160 KB rule of chv_scale_lanczos on the plane's own sizes against the TARGET's), then makes ONE "launch", which
// asks the runtime once whether it should fail.  A launch is a closure on the stream that, when the stream gets to it, reads the first and
// last entry of all four tables, the first and last byte of EVERY source plane of every picture and touches the first and last byte of
// every target — the planes read LATE, from the descriptor slot for a batch and from the job for a lone call: a table freed while a launch
// still needs it, a slot overwritten too early or laid out with the wrong record length, a picture freed under a queued launch or a plane
// whose extent was not checked is a sanitizer report.  A target's first byte counts the launches that wrote it.
#include <hip/hip_runtime.h>

#include "../../swiftvideo_amd/csrc/lanczos_from_yuv.h"
#include "stub_lanczos_refuses.h"

namespace chv {
static hipError_t stub_lanczos_from_yuv(const LanczosFromYuvJob &job_in, hipStream_t stream) {
    const int snp = job_in.src_planes;
    if ((snp != 2 && snp != 3) || job_in.n_pictures < 1 || (job_in.n_pictures > 1 && !job_in.batch)) return hipErrorInvalidValue;
    if (job_in.rgba != 0 && job_in.rgba != 1) return hipErrorInvalidValue;
    if (job_in.cy != 76309 && job_in.cy != 65536) return hipErrorInvalidValue;        // (one of section 4.2's rows arrived)
    for (int p = 0; p < 2; p++) {
        const LanczosPlaneTables &t = p ? job_in.chroma : job_in.luma;
        const DPlane &s = job_in.src[p];
        if (job_in.dst.w < 1 || job_in.dst.h < 1 || s.w < 1 || s.h < 1 || stub_lanczos_refuses(job_in.dst.w, job_in.dst.h, s.w, s.h, t.tx, t.ty))
            return hipErrorInvalidValue;
    }
    if (stubhip_launch_should_fail()) return hipErrorLaunchFailure;
    const LanczosFromYuvJob job = job_in;
    stubhip_enqueue(stream, [job] {
        volatile float sink = 0.f;
        const int snp = job.src_planes;
        const size_t per = (size_t)1 + snp;
        for (int p = 0; p < 2; p++) {
            const LanczosPlaneTables &t = p ? job.chroma : job.luma;
            sink = sink + (float)t.fx[0] + (float)t.fx[job.dst.w - 1] + t.wx[0] + t.wx[(size_t)job.dst.w * t.tx - 1];
            sink = sink + (float)t.fy[0] + (float)t.fy[job.dst.h - 1] + t.wy[0] + t.wy[(size_t)job.dst.h * t.ty - 1];
        }
        for (int i = 0; i < job.n_pictures; i++) {
            unsigned sum = 0;
            for (int q = 0; q < snp; q++) {
                const DPlane s = job.batch ? job.batch[(size_t)i * per + 1 + q] : job.src[q];
                const volatile uint8_t *sp = s.ptr;
                sum += sp[0] + sp[(size_t)(s.h - 1) * s.pitch + (size_t)s.w * s.comps - 1];
            }
            const DPlane d = job.batch ? job.batch[(size_t)i * per] : job.dst;
            volatile uint8_t *dp = d.ptr;
            const size_t last = (size_t)(d.h - 1) * d.pitch + (size_t)d.w * d.comps - 1;
            dp[0] = (uint8_t)(dp[0] + 1);
            if (last) dp[last] = (uint8_t)(0xA5 ^ (sum & 1));
        }
    });
    return hipSuccess;
}
static const struct LanczosFromYuvRegistrar { LanczosFromYuvRegistrar() { register_lanczos_from_yuv_launcher(stub_lanczos_from_yuv); } } g_lanczos_from_yuv_registrar;
}  // namespace chv
