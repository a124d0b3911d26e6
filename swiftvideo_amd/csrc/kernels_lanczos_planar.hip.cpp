// kernels_lanczos_planar.hip.cpp — separable Lanczos-3 resampler for the planes of 4:2:0 pictures: 1-component planes (luma, the Cb and Cr
// planes of y420p) and the 2-component CbCr plane of NV12.  Plane-wise: every plane is an image of its own, resampled
// with the tables of its own width and height, every component through the chain of kernels_lanczos.hip.cpp (horizontal then vertical pass,
// one fused multiply-add per tap from 0.0f, taps ascending, float intermediate, convert_uchar_sat_rte).  No colour arithmetic.
//
// ONE launch covers every plane of a picture and every picture of a batch chunk: a block's number decodes to (picture, plane, row chunk,
// strip), and every plane brings its own tables and tap counts.
//
// The row code of both kernels — planar_strip<T, C>: one wave per strip of 64 output bytes, tap counts up to 22; planar_tile: everything else —
// and the host rules (route, launch numbers, refusal) are in lanczos_planar_body.hip.h, shared with the ladder unit
// (kernels_lanczos_planar_ladder.hip.cpp).  Here:
//
//   planar_lanczos_strip<T>  every plane's tap counts <= T <= 22 and a staged row of at most 64 vectors: planar_strip<T, C> per block
//   planar_lanczos_tile      everything else (more than 22 taps on some axis of some plane): planar_tile per block
#include "lanczos_planar_body.hip.h"

namespace chv {

struct PlanarArgs {
    PlanarPlane pl[kLanczosPlanarMaxPlanes];
    const DPlane *batch;
    int32_t n_planes, rows;           // rows: output rows per wave (strip kernel)
    int32_t per_picture, total;       // blocks per picture, blocks in all
};
static_assert(sizeof(PlanarArgs) <= 1024, "kernel arguments: 4 KB in all");

struct PlanarBlock {
    PlanarPlane g;
    int picture, bx, by;
};

// (picture, plane, row chunk, strip) of block `idx`; dst / src of a batch come from the descriptor list
CHV_DEV PlanarBlock planar_decode(int idx) {
    const uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const int n_planes = cld<int32_t>(ka + offsetof(PlanarArgs, n_planes));
    const int per = cld<int32_t>(ka + offsetof(PlanarArgs, per_picture));
    const uint64_t batch = cld<uint64_t>(ka + offsetof(PlanarArgs, batch));
    PlanarBlock r;
    r.picture = idx / per;
    const int rem = idx - r.picture * per;
    const int f1 = cld<int32_t>(ka + offsetof(PlanarArgs, pl) + sizeof(PlanarPlane) + offsetof(PlanarPlane, first));
    const int f2 = cld<int32_t>(ka + offsetof(PlanarArgs, pl) + 2 * sizeof(PlanarPlane) + offsetof(PlanarPlane, first));
    const int plane = (n_planes > 2 && rem >= f2) ? 2 : rem >= f1 ? 1 : 0;
    r.g = cld<PlanarPlane>(ka + offsetof(PlanarArgs, pl) + (uint64_t)plane * sizeof(PlanarPlane));
    const int in_plane = rem - r.g.first;
    r.by = in_plane / r.g.strips;
    r.bx = in_plane - r.by * r.g.strips;
    if (batch) {
        const uint64_t pair = batch + ((uint64_t)r.picture * n_planes + plane) * 2 * sizeof(DPlane);
        r.g.dst = cld<DPlane>(pair); r.g.src = cld<DPlane>(pair + sizeof(DPlane));
    }
    return r;
}

template <int T>
__global__ __launch_bounds__(64, (T <= 12 ? 5 : 4)) void planar_lanczos_strip(const PlanarArgs a) {
    // XCD-aware numbering, as in lanczos3_strip2: block b runs on XCD b % 8, and every XCD gets one contiguous range of (picture, plane,
    // row chunk, strip) — neighbouring strips and chunks share their halo columns and rows through that XCD's L2
    const int b = blockIdx.x, per_xcd = (a.total + 7) >> 3;
    const int idx = (b & 7) * per_xcd + (b >> 3);
    if ((b >> 3) >= per_xcd || idx >= a.total) return;
    extern __shared__ __attribute__((aligned(16))) uint8_t planar_lsm[];
    const PlanarBlock blk = planar_decode(idx);
    if (blk.g.dst.comps == 2) planar_strip<T, 2>(blk.g, blk.bx, blk.by, a.rows, planar_lsm);
    else planar_strip<T, 1>(blk.g, blk.bx, blk.by, a.rows, planar_lsm);
}

__global__ __launch_bounds__(256) void planar_lanczos_tile(const PlanarArgs a) {
    const int idx = blockIdx.x;
    if (idx >= a.total) return;
    extern __shared__ __attribute__((aligned(16))) uint8_t planar_lsm[];
    const PlanarBlock blk = planar_decode(idx);
    planar_tile(blk.g, blk.bx, blk.by, planar_lsm);
}

static hipError_t launch_lanczos_planar(const LanczosPlanarJob &job, hipStream_t stream) {
    if (job.n_planes < 2 || job.n_planes > kLanczosPlanarMaxPlanes || job.n_pictures < 1) return hipErrorInvalidValue;
    PlanarArgs a{};
    a.batch = job.batch;
    a.n_planes = job.n_planes;
    for (int p = 0; p < job.n_planes; p++) {
        const LanczosPlaneTables &t = job.tab[p];
        const DPlane &d = job.dst[p], &s = job.src[p];
        if (d.comps != s.comps || (d.comps != 1 && d.comps != 2)) return hipErrorInvalidValue;
        if (lanczos_refuses(d.w, d.h, s.w, s.h, t.tx, t.ty)) return hipErrorInvalidValue;        // any plane refused: nothing is launched
        PlanarPlane &g = a.pl[p];
        g.fx = t.fx; g.wx = t.wx; g.fy = t.fy; g.wy = t.wy; g.tx = t.tx; g.ty = t.ty;
        g.dst = d; g.src = s;
    }
    int T = 0, nvmax = 0;
    const bool strip_route = planar_strip_route(a.pl, job.n_planes, &T, &nvmax);      // (lanczos_route.h: the rule, shared with the ladder)
    (void)hipGetLastError();
    if (strip_route) {
        a.rows = lanczos_strip_rows(planar_strip_work(a.pl, job.n_planes) * job.n_pictures, PS_MAX_ROWS);
        a.per_picture = planar_strip_blocks(a.pl, job.n_planes, a.rows);
        const long total = (long)a.per_picture * job.n_pictures;
        if (total > 0x3fffffff) return hipErrorInvalidValue;
        a.total = (int)total;
        dim3 grid((unsigned)(((a.total + 7) / 8) * 8));
        const size_t lds = lanczos_wtab_bytes(a.rows, T) + (size_t)2 * nvmax * 16;       // the strip's vertical weights, the two-row staging ring
        switch (T) {
        case 6: hipLaunchKernelGGL(planar_lanczos_strip<6>, grid, dim3(64), lds, stream, a); break;
        case 8: hipLaunchKernelGGL(planar_lanczos_strip<8>, grid, dim3(64), lds, stream, a); break;
        case 12: hipLaunchKernelGGL(planar_lanczos_strip<12>, grid, dim3(64), lds, stream, a); break;
        case 16: hipLaunchKernelGGL(planar_lanczos_strip<16>, grid, dim3(64), lds, stream, a); break;
        default: hipLaunchKernelGGL(planar_lanczos_strip<22>, grid, dim3(64), lds, stream, a); break;
        }
        return hipGetLastError();
    }
    int rows_max = 0;
    a.per_picture = planar_tile_blocks(a.pl, job.n_planes, &rows_max);
    const long total = (long)a.per_picture * job.n_pictures;
    if (total > 0x3fffffff) return hipErrorInvalidValue;
    a.total = (int)total;
    const size_t lds = (size_t)rows_max * PT_W * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;                // (not reached: 256 taps and the refusal above bound it by 50 KB)
    hipLaunchKernelGGL(planar_lanczos_tile, dim3((unsigned)a.total), dim3(256), lds, stream, a);
    return hipGetLastError();
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosPlanarRegistrar { LanczosPlanarRegistrar() { register_lanczos_planar_launcher(launch_lanczos_planar); } } g_lanczos_planar_registrar;

}  // namespace chv
