// tests/stubhip/stub_lanczos_ladder_launcher.cpp — the stand-in for kernels_lanczos_ladder.hip.cpp in the sanitizer builds
// (tests/test_lanczos_ladder_sanitizers.py).  TEST INFRASTRUCTURE.  Like the unit it stands for, it checks every rung before anything is
// enqueued (the 160 KB rule of chv_scale_lanczos), then makes ONE "launch" for the rungs with equal, even tap counts 6 .. 22 and one more for
// the others — each asks the runtime once whether it should fail.  A launch is a closure on the stream that, when the stream gets to it, reads
// the first and last entry of each of its rungs' tables and touches the first and last byte of those rungs' planes of every picture, read LATE
// from the descriptor slot: a table freed while a launch still needs it, a slot overwritten too early, a picture freed under a queued launch or
// a plane whose extent was not checked is a sanitizer report.  Every target plane's first byte counts the launches that wrote it.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../swiftvideo_amd/csrc/lanczos_ladder.h"
#include "stub_lanczos_refuses.h"

namespace chv {
static hipError_t stub_lanczos_ladder(const LanczosLadderJob &job_in, hipStream_t stream, int *launches) {
    *launches = 0;
    if ((job_in.n_dst != 2 && job_in.n_dst != 3) || job_in.n_pictures < 1 || job_in.n_rungs < 1 || job_in.n_rungs > kLanczosLadderMaxRungs || !job_in.batch)
        return hipErrorInvalidValue;
    // (the matrix arrives in the source's byte order: rows that sum to the luma gain and to zero whatever the order is)
    if (job_in.ku[0] + job_in.ku[1] + job_in.ku[2] != 0 || job_in.kv[0] + job_in.kv[1] + job_in.kv[2] != 0 || job_in.ky[1] < job_in.ky[0]) return hipErrorInvalidValue;
    std::vector<int> route[2];
    for (int r = 0; r < job_in.n_rungs; r++) {
        const LanczosLadderRung &g = job_in.rung[r];
        if (stub_lanczos_refuses(g.w, g.h, job_in.src_w, job_in.src_h, g.tx, g.ty)) return hipErrorInvalidValue;
        route[g.tx == g.ty && g.tx >= 6 && g.tx <= 22 && (g.tx & 1) == 0 ? 0 : 1].push_back(r);
    }
    const LanczosLadderJob job = job_in;
    for (const std::vector<int> &rungs : route) {
        if (rungs.empty()) continue;
        if (stubhip_launch_should_fail()) return hipErrorLaunchFailure;
        stubhip_enqueue(stream, [job, rungs] {
            volatile float sink = 0.f;
            const size_t per = (size_t)job.n_rungs * job.n_dst + 1;
            for (int r : rungs) {
                const LanczosLadderRung &g = job.rung[r];
                sink = sink + (float)g.fx[0] + (float)g.fx[g.w - 1] + g.wx[0] + g.wx[(size_t)g.w * g.tx - 1];
                sink = sink + (float)g.fy[0] + (float)g.fy[g.h - 1] + g.wy[0] + g.wy[(size_t)g.h * g.ty - 1];
                for (int i = 0; i < job.n_pictures; i++) {
                    const DPlane s = job.batch[(size_t)i * per + per - 1];
                    const volatile uint8_t *sp = s.ptr;
                    const unsigned sum = sp[0] + sp[(size_t)(s.h - 1) * s.pitch + (size_t)s.w * s.comps - 1];
                    for (int p = 0; p < job.n_dst; p++) {
                        const DPlane d = job.batch[(size_t)i * per + (size_t)r * job.n_dst + p];
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
static const struct LadderRegistrar { LadderRegistrar() { register_lanczos_ladder_launcher(stub_lanczos_ladder); } } g_ladder_registrar;
}  // namespace chv
