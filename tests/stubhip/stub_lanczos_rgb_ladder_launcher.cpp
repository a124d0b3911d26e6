// tests/stubhip/stub_lanczos_rgb_ladder_launcher.cpp — the stand-in for kernels_lanczos_rgb_ladder.hip.cpp in the sanitizer builds
// (tests/test_lanczos_rgb_ladder_sanitizers.py).  TEST INFRASTRUCTURE.  Like the unit it stands for, it checks EVERY rung before anything is
// enqueued (the 160 KB rule of chv_scale_lanczos on the rung's sizes), then makes one "launch" for the rungs of the strip route (no axis
// beyond 22 taps, a source of at least 4 texels, a staged row of at most 64 vectors) and one more for the others, each of which asks the
// runtime once whether it should fail.  A launch is a closure on the stream that, when the stream gets to it, reads the first and last
// entry of both tables of each of its rungs, the first and last byte of the source plane of every picture and touches the first and last
// byte of every target of its rungs — the planes read LATE, from the descriptor slot: a table freed while a launch still needs it, a slot
// overwritten too early or laid out with the wrong record length, a picture freed under a queued launch or a plane whose extent was not
// checked is a sanitizer report.  A target's first byte counts the launches that wrote it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../swiftvideo_amd/csrc/lanczos_rgb_ladder.h"
#include "stub_lanczos_refuses.h"

namespace chv {
static bool stub_rgb_ladder_tile(const LanczosRgbLadderJob &job, const LanczosRgbLadderRung &R) {
    const int nv = ((int)(63 * ((double)job.src_w / (double)R.w)) + 1 + 3 + R.tab.tx + 3) / 4 + 1;
    return !(std::max(R.tab.tx, R.tab.ty) <= 22 && job.src_w >= 4 && nv <= 64);
}

static hipError_t stub_lanczos_rgb_ladder(const LanczosRgbLadderJob &job_in, hipStream_t stream, int *launches) {
    *launches = 0;
    if (job_in.n_pictures < 1 || !job_in.batch || job_in.n_rungs < 1 || job_in.n_rungs > kLanczosPlanarLadderMaxRungs) return hipErrorInvalidValue;
    bool route[2] = { false, false };
    for (int r = 0; r < job_in.n_rungs; r++) {
        const LanczosRgbLadderRung &R = job_in.rung[r];
        if (R.w < 1 || R.h < 1 || job_in.src_w < 1 || job_in.src_h < 1 || stub_lanczos_refuses(R.w, R.h, job_in.src_w, job_in.src_h, R.tab.tx, R.tab.ty))
            return hipErrorInvalidValue;
        route[stub_rgb_ladder_tile(job_in, R)] = true;
    }
    for (int tile = 0; tile < 2; tile++) {
        if (!route[tile]) continue;
        if (stubhip_launch_should_fail()) return hipErrorLaunchFailure;
        const LanczosRgbLadderJob job = job_in;
        stubhip_enqueue(stream, [job, tile] {
            volatile float sink = 0.f;
            const size_t per = (size_t)job.n_rungs + 1;
            for (int r = 0; r < job.n_rungs; r++) {
                const LanczosRgbLadderRung &R = job.rung[r];
                if (stub_rgb_ladder_tile(job, R) != (tile != 0)) continue;
                const LanczosPlaneTables &t = R.tab;
                sink = sink + (float)t.fx[0] + (float)t.fx[R.w - 1] + t.wx[0] + t.wx[(size_t)R.w * t.tx - 1];
                sink = sink + (float)t.fy[0] + (float)t.fy[R.h - 1] + t.wy[0] + t.wy[(size_t)R.h * t.ty - 1];
                for (int i = 0; i < job.n_pictures; i++) {
                    const DPlane s = job.batch[(size_t)i * per + job.n_rungs];
                    const volatile uint8_t *sp = s.ptr;
                    const unsigned sum = sp[0] + sp[(size_t)(s.h - 1) * s.pitch + (size_t)s.w * s.comps - 1];
                    const DPlane d = job.batch[(size_t)i * per + r];
                    volatile uint8_t *dp = d.ptr;
                    const size_t last = (size_t)(d.h - 1) * d.pitch + (size_t)d.w * d.comps - 1;
                    dp[0] = (uint8_t)(dp[0] + 1);
                    if (last) dp[last] = (uint8_t)(0xA5 ^ (sum & 1));
                }
            }
        });
        ++*launches;
    }
    return hipSuccess;
}
static const struct LanczosRgbLadderRegistrar {
    LanczosRgbLadderRegistrar() { register_lanczos_rgb_ladder_launcher(stub_lanczos_rgb_ladder); }
} g_lanczos_rgb_ladder_registrar;
}  // namespace chv
