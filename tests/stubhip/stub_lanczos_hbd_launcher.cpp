// tests/stubhip/stub_lanczos_hbd_launcher.cpp — the stand-in for kernels_lanczos_hbd.hip.cpp in the sanitizer builds
// (tests/test_lanczos_hbd_sanitizers.py).  TEST INFRASTRUCTURE.  Like the unit it stands for, it checks every logical image of every rung
// before anything is enqueued (the 160 KB rule of chv_scale_lanczos), then makes ONE "launch" for the rungs whose images all have at most 22
// taps on both axes and one more for the others — each asks the runtime once whether it should fail.  A launch is a closure on the stream
// that, when the stream gets to it, reads the first and last entry of every table of each of its rungs' target planes, the first and last
// 16-BIT WORD of every source plane of every picture (so a plane at an odd address or with an odd pitch is a misaligned load under UBSan) and
// touches the first and last byte of those rungs' target planes, read LATE from the descriptor slot: a table freed while a launch still needs
// it, a slot overwritten too early or laid out with the wrong record length, a picture freed under a queued launch or a plane whose extent was
// not checked is a sanitizer report.  Every target plane's first byte counts the launches that wrote it.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../swiftvideo_amd/csrc/lanczos_hbd.h"
#include "stub_lanczos_refuses.h"

namespace chv {
static hipError_t stub_lanczos_hbd(const LanczosHbdJob &job_in, hipStream_t stream, int *launches) {
    *launches = 0;
    const int np = job_in.dst_planes, snp = job_in.src_planes;
    if ((np != 2 && np != 3) || (job_in.source != kHbdP010 && job_in.source != kHbdPlanar) || snp != (job_in.source == kHbdP010 ? 2 : 3) ||
        job_in.n_pictures < 1 || job_in.n_rungs < 1 || job_in.n_rungs > kLanczosPlanarLadderMaxRungs || !job_in.batch)
        return hipErrorInvalidValue;
    std::vector<int> route[2];
    for (int r = 0; r < job_in.n_rungs; r++) {
        const Lanczos420Rung &g = job_in.rung[r];
        bool strip = true;
        for (int p = 0; p < np; p++) {
            const int sw = p ? job_in.chroma_w : job_in.luma_w, sh = p ? job_in.chroma_h : job_in.luma_h;
            if (g.w[p] < 1 || g.h[p] < 1 || sw < 1 || sh < 1 || stub_lanczos_refuses(g.w[p], g.h[p], sw, sh, g.tab[p].tx, g.tab[p].ty)) return hipErrorInvalidValue;
            if (g.tab[p].tx > 22 || g.tab[p].ty > 22) strip = false;
        }
        route[strip ? 0 : 1].push_back(r);
    }
    const LanczosHbdJob job = job_in;
    for (const std::vector<int> &rungs : route) {
        if (rungs.empty()) continue;
        if (stubhip_launch_should_fail()) return hipErrorLaunchFailure;
        stubhip_enqueue(stream, [job, rungs] {
            volatile float sink = 0.f;
            const int np = job.dst_planes, snp = job.src_planes;
            const size_t per = (size_t)job.n_rungs * np + snp, src_at = (size_t)job.n_rungs * np;
            for (int r : rungs) {
                const Lanczos420Rung &g = job.rung[r];
                for (int p = 0; p < np; p++) {
                    const LanczosPlaneTables &t = g.tab[p];
                    sink = sink + (float)t.fx[0] + (float)t.fx[g.w[p] - 1] + t.wx[0] + t.wx[(size_t)g.w[p] * t.tx - 1];
                    sink = sink + (float)t.fy[0] + (float)t.fy[g.h[p] - 1] + t.wy[0] + t.wy[(size_t)g.h[p] * t.ty - 1];
                    for (int i = 0; i < job.n_pictures; i++) {
                        unsigned sum = 0;
                        for (int q = 0; q < snp; q++) {
                            const DPlane s = job.batch[(size_t)i * per + src_at + q];
                            const volatile uint16_t *first = (const volatile uint16_t *)s.ptr;
                            const volatile uint16_t *last = (const volatile uint16_t *)(s.ptr + (size_t)(s.h - 1) * s.pitch + (size_t)s.w * s.comps - 2);
                            sum += *first + *last;
                        }
                        const DPlane d = job.batch[(size_t)i * per + (size_t)r * np + p];
                        volatile uint8_t *dp = d.ptr;
                        const size_t last = (size_t)(d.h - 1) * d.pitch + (size_t)d.w * d.comps - 1;
                        dp[0] = (uint8_t)(dp[0] + 1);
                        if (last) dp[last] = (uint8_t)(0xA5 ^ (sum & 1));
                    }
                }
            }
        });
        ++*launches;
    }
    return hipSuccess;
}
static const struct LanczosHbdRegistrar { LanczosHbdRegistrar() { register_lanczos_hbd_launcher(stub_lanczos_hbd); } } g_lanczos_hbd_registrar;
}  // namespace chv
