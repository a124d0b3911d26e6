// kernels_lanczos_ladder.hip.cpp — every rung of an encoder ladder in one launch (no reference counterpart): the
// renditions of one or several BGRA / RGBA canvases of one size as NV12 or y420p pictures of up to eight sizes.  The row code is that of
// chv_scale_lanczos_to_yuv (lanczos_to_yuv_body.hip.h), so the bytes are; what is new is how a block finds its work.
//
//   lanczos_yuv_ladder<MAXT>   the rungs that take the wave-per-strip route.  ONE grid of 64-thread blocks, the concatenation of the rungs' block
//                              ranges, largest rung first (the grid's tail is made of the small rungs' blocks).  A block finds its rung by a scalar
//                              scan of the cumulative block counts in the arguments, then its picture, row chunk and strip as lanczos_yuv_strip<T>
//                              does — with the XCD-aware numbering run PER RUNG: every range starts on a multiple of 8 and is padded to one, so
//                              blocks of equal b & 7 still share an XCD and neighbouring strips of one picture of one rung stay on one — reads its
//                              planes from the descriptor list through the scalar unit, and dispatches (uniformly) on the rung's tap count to the
//                              shared strip body.  A kernel is allocated the registers of its largest body, hence two variants by the largest
//                              tap count among the ladder's strip rungs: <16> holds the bodies of 6 .. 16 taps at four waves per SIMD, <22>
//                              all nine at three (the bodies from 18 taps on in their lean form).
//   lanczos_yuv_ladder_tile    the rungs that take the tile route, the same construction over the shared tile body: 256-thread blocks, one per
//                              tw x 4 tile.
//
// Dynamic LDS is the maximum over the launch's rungs.
#include "lanczos_to_yuv_body.hip.h"
#include "lanczos_ladder.h"
#include "lanczos_ladder_launch.hip.h"

namespace chv {

struct LadderRung {
    const int32_t *fx; const float *wx;
    const int32_t *fy; const float *wy;
    int32_t tx, ty;                   // taps (strip route: tx == ty == T)
    int32_t nv, rows;                 // strip route: vectors of a staged row, output rows per wave (even)
    int32_t tw, max_rows;             // tile route: tile width (32 or 8), rows of the LDS array
    int32_t strips, chunks;           // blocks along x and y of one picture
    int32_t per_picture, total;       // blocks per picture, blocks of all pictures (the range in the grid: `total` rounded up to 8 for strips)
    int32_t first_block;              // where the rung's range starts in the grid
    int32_t dst_at;                   // the rung's first target plane within a picture's descriptor
};

struct LadderArgs {
    const DPlane *batch;              // per picture: n_rungs * n_dst target planes, then the source plane
    int32_t n_dst, per_image;         // planes of a target, planes of a picture's descriptor
    int32_t ybase, ky0, ky1, ky2, ku0, ku1, ku2, kv0, kv1, kv2;      // ybase = (yoff << 16) + 32768
    int32_t first[kLanczosLadderMaxRungs];      // first_block of rung k of this launch (INT_MAX beyond the last): what the scan reads
    LadderRung rung[kLanczosLadderMaxRungs];
};
static_assert(sizeof(LadderArgs) <= 1024, "kernel arguments: 4 KB in all");
static_assert(kLanczosLadderMaxRungs == kLanczosPlanarLadderMaxRungs, "lanczos_ladder_grid.h scans and orders this many rungs");

// picture `image`'s planes for the rung whose targets start at plane `dst_at`: from the descriptor list (scalar loads)
CHV_DEV ToYuvPlanes ladder_planes(const LadderArgs &a, int image, int dst_at) {
    const uint64_t pic = (uint64_t)(uintptr_t)a.batch + (uint64_t)image * a.per_image * sizeof(DPlane);
    const uint64_t at = pic + (uint64_t)dst_at * sizeof(DPlane);
    ToYuvPlanes p;
    p.y = cld<DPlane>(at);
    p.c0 = cld<DPlane>(at + sizeof(DPlane));
    p.c1 = cld<DPlane>(at + (a.n_dst == 3 ? 2 : 1) * sizeof(DPlane));
    p.src = cld<DPlane>(pic + (uint64_t)(a.per_image - 1) * sizeof(DPlane));
    return p;
}

template <int MAXT>
__global__ __launch_bounds__(64, (MAXT >= 18 ? 3 : 4)) void lanczos_yuv_ladder(const LadderArgs a) {
    const int r = ladder_rung_of(a.first, blockIdx.x);
    const LadderRung &R = a.rung[r];
    const LadderItem it = ladder_item<true>(blockIdx.x - R.first_block, R.total);      // XCD-aware numbering inside the rung's range
    if (!it.live) return;
    const int idx = it.idx;
    const int per_picture = R.per_picture, strips = R.strips;
    const int image = idx / per_picture, rem = idx - image * per_picture;
    const int chunk = rem / strips, strip = rem - chunk * strips;
    const ToYuvPlanes P = ladder_planes(a, image, R.dst_at);
#define CHV_LL_CASE(TT) case TT: if constexpr (TT <= MAXT) lanczos_yuv_strip_body<TT, true>(a, P, R, chunk, strip); break
    switch (R.tx) {                   // (uniform)
    CHV_LL_CASE(6); CHV_LL_CASE(8); CHV_LL_CASE(10); CHV_LL_CASE(12); CHV_LL_CASE(14); CHV_LL_CASE(16); CHV_LL_CASE(18); CHV_LL_CASE(20); CHV_LL_CASE(22);
    default: break;
    }
#undef CHV_LL_CASE
}

__global__ __launch_bounds__(256) void lanczos_yuv_ladder_tile(const LadderArgs a) {
    const int r = ladder_rung_of(a.first, blockIdx.x);
    const LadderRung &R = a.rung[r];
    const LadderItem it = ladder_item<false>(blockIdx.x - R.first_block, R.total);
    if (!it.live) return;
    const int idx = it.idx;
    const int per_picture = R.per_picture, strips = R.strips;
    const int image = idx / per_picture, rem = idx - image * per_picture;
    const int by = rem / strips, bx = rem - by * strips;
    const ToYuvPlanes P = ladder_planes(a, image, R.dst_at);
    lanczos_yuv_tile_body(a, P, R, by, bx);
}

static hipError_t launch_lanczos_ladder(const LanczosLadderJob &job, hipStream_t stream, int *launches) {
    *launches = 0;
    if ((job.n_dst != 2 && job.n_dst != 3) || job.n_pictures < 1 || job.n_rungs < 1 || job.n_rungs > kLanczosLadderMaxRungs || !job.batch) return hipErrorInvalidValue;
    // every rung's route and numbers before anything is launched: one refused rung refuses the ladder
    LadderRung strip[kLanczosLadderMaxRungs], tile[kLanczosLadderMaxRungs];
    int n_strip = 0, n_tile = 0, max_t = 0;
    size_t strip_lds = 0, tile_lds = 0;
    long work = 0;
    for (int r = 0; r < job.n_rungs; r++) {
        const LanczosLadderRung &j = job.rung[r];
        if (j.w < 1 || j.h < 1 || lanczos_refuses(j.w, j.h, job.src_w, job.src_h, j.tx, j.ty)) return hipErrorInvalidValue;
        LadderRung R{};
        R.fx = j.fx; R.wx = j.wx; R.fy = j.fy; R.wy = j.wy; R.tx = j.tx; R.ty = j.ty;
        R.dst_at = r * job.n_dst;
        if (const int nv = to_yuv_strip_vectors(j.w, job.src_w, j.tx, j.ty)) {
            R.nv = nv;
            R.strips = (j.w + 63) / 64;
            R.chunks = j.h;                             // (the output rows, until `rows` is known)
            work += (long)j.h * R.strips * job.n_pictures;
            max_t = std::max(max_t, (int)j.tx);
            strip_lds = std::max(strip_lds, (size_t)2 * nv * 16);
            strip[n_strip++] = R;
        } else {
            const size_t lds = to_yuv_tile_shape(j.h, job.src_h, j.ty, &R.tw, &R.max_rows);
            if (lds > 64 * 1024) return hipErrorInvalidValue;
            R.strips = (j.w + R.tw - 1) / R.tw;
            R.chunks = (j.h + YT_H - 1) / YT_H;
            R.per_picture = R.strips * R.chunks;
            const long total = (long)R.per_picture * job.n_pictures;
            if (total > 0x3fffffff) return hipErrorInvalidValue;
            R.total = (int32_t)total;
            tile_lds = std::max(tile_lds, lds);
            tile[n_tile++] = R;
        }
    }
    // rows per wave from the whole ladder's strip work (lanczos_yuv_strip<T>'s rule over the sum): one count for every rung
    const int rows = to_yuv_strip_rows(work);
    for (int k = 0; k < n_strip; k++) {
        LadderRung &R = strip[k];
        R.rows = rows;
        R.chunks = (R.chunks + rows - 1) / rows;
        R.per_picture = R.strips * R.chunks;
        const long total = (long)R.per_picture * job.n_pictures;
        if (total > 0x3fffffff) return hipErrorInvalidValue;
        R.total = (int32_t)total;
    }
    LadderArgs a{};
    a.batch = job.batch; a.n_dst = job.n_dst; a.per_image = job.n_rungs * job.n_dst + 1;
    a.ybase = (job.yoff << 16) + 32768;
    a.ky0 = job.ky[0]; a.ky1 = job.ky[1]; a.ky2 = job.ky[2];
    a.ku0 = job.ku[0]; a.ku1 = job.ku[1]; a.ku2 = job.ku[2];
    a.kv0 = job.kv[0]; a.kv1 = job.kv[1]; a.kv2 = job.kv[2];
    LadderArgs t = a;
    unsigned strip_grid = 0, tile_grid = 0;
    if (n_strip && !ladder_order(&a, strip, n_strip, 8, &strip_grid)) return hipErrorInvalidValue;
    if (n_tile && !ladder_order(&t, tile, n_tile, 1, &tile_grid)) return hipErrorInvalidValue;
    return ladder_launch(launches, n_strip, [&] {
        if (max_t <= 16) hipLaunchKernelGGL(lanczos_yuv_ladder<16>, dim3(strip_grid), dim3(64), strip_lds, stream, a);
        else hipLaunchKernelGGL(lanczos_yuv_ladder<22>, dim3(strip_grid), dim3(64), strip_lds, stream, a);
    }, n_tile, [&] { hipLaunchKernelGGL(lanczos_yuv_ladder_tile, dim3(tile_grid), dim3(256), tile_lds, stream, t); });
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosLadderRegistrar { LanczosLadderRegistrar() { register_lanczos_ladder_launcher(launch_lanczos_ladder); } } g_lanczos_ladder_registrar;

}  // namespace chv
