// tests/stubhip/stub_lanczos_from_yuv_ladder_launcher.cpp — the stand-in for kernels_lanczos_from_yuv_ladder.hip.cpp in the sanitizer builds
// (tests/test_lanczos_from_yuv_ladder_sanitizers.py).  TEST INFRASTRUCTURE.  Like the unit it stands for, it checks both logical planes of
// EVERY rung before anything is enqueued (the 160 KB rule of chv_scale_lanczos on the plane's own sizes against the rung's), then makes one
// "launch" for the rungs of at most 22 taps and one more for the others, each of which asks the runtime once whether it should fail.  A
// launch is a closure on the stream that, when the stream gets to it, reads the first and last entry of all four tables of each of its
// rungs, the first and last byte of EVERY source plane of every picture and touches the first and last byte of every target of its rungs —
// the planes read LATE, from the descriptor slot: a table freed while a launch still needs it, a slot overwritten too early or laid out
// with the wrong record length, a picture freed under a queued launch or a plane whose extent was not checked is a sanitizer report.  A
// target's first byte counts the launches that wrote it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../swiftvideo_amd/csrc/lanczos_from_yuv_ladder.h"
#include "stub_lanczos_refuses.h"

namespace chv {
static hipError_t stub_lanczos_from_yuv_ladder(const LanczosFromYuvLadderJob &job_in, hipStream_t stream, int *launches) {
    *launches = 0;
    const int snp = job_in.src_planes;
    if ((snp != 2 && snp != 3) || job_in.n_pictures < 1 || !job_in.batch || job_in.n_rungs < 1 || job_in.n_rungs > kLanczosPlanarLadderMaxRungs)
        return hipErrorInvalidValue;
    if (job_in.rgba != 0 && job_in.rgba != 1) return hipErrorInvalidValue;
    if (job_in.cy != 76309 && job_in.cy != 65536) return hipErrorInvalidValue;        // (one of section 4.2's rows arrived)
    bool route[2] = { false, false };
    for (int r = 0; r < job_in.n_rungs; r++) {
        const LanczosFromYuvLadderRung &R = job_in.rung[r];
        int tmax = 0;
        for (int p = 0; p < 2; p++) {
            const LanczosPlaneTables &t = p ? R.chroma : R.luma;
            const int sw = p ? job_in.chroma_w : job_in.luma_w, sh = p ? job_in.chroma_h : job_in.luma_h;
            if (R.w < 1 || R.h < 1 || sw < 1 || sh < 1 || stub_lanczos_refuses(R.w, R.h, sw, sh, t.tx, t.ty)) return hipErrorInvalidValue;
            tmax = std::max(tmax, std::max(t.tx, t.ty));
        }
        route[tmax > 22] = true;
    }
    for (int tile = 0; tile < 2; tile++) {
        if (!route[tile]) continue;
        if (stubhip_launch_should_fail()) return hipErrorLaunchFailure;
        const LanczosFromYuvLadderJob job = job_in;
        stubhip_enqueue(stream, [job, tile] {
            volatile float sink = 0.f;
            const int snp = job.src_planes;
            const size_t per = (size_t)job.n_rungs + snp;
            for (int r = 0; r < job.n_rungs; r++) {
                const LanczosFromYuvLadderRung &R = job.rung[r];
                if ((std::max(std::max(R.luma.tx, R.luma.ty), std::max(R.chroma.tx, R.chroma.ty)) > 22) != (tile != 0)) continue;
                for (int p = 0; p < 2; p++) {
                    const LanczosPlaneTables &t = p ? R.chroma : R.luma;
                    sink = sink + (float)t.fx[0] + (float)t.fx[R.w - 1] + t.wx[0] + t.wx[(size_t)R.w * t.tx - 1];
                    sink = sink + (float)t.fy[0] + (float)t.fy[R.h - 1] + t.wy[0] + t.wy[(size_t)R.h * t.ty - 1];
                }
                for (int i = 0; i < job.n_pictures; i++) {
                    unsigned sum = 0;
                    for (int q = 0; q < snp; q++) {
                        const DPlane s = job.batch[(size_t)i * per + job.n_rungs + q];
                        const volatile uint8_t *sp = s.ptr;
                        sum += sp[0] + sp[(size_t)(s.h - 1) * s.pitch + (size_t)s.w * s.comps - 1];
                    }
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
static const struct LanczosFromYuvLadderRegistrar {
    LanczosFromYuvLadderRegistrar() { register_lanczos_from_yuv_ladder_launcher(stub_lanczos_from_yuv_ladder); }
} g_lanczos_from_yuv_ladder_registrar;
}  // namespace chv
