// kernels_lanczos_rgb_ladder.hip.cpp — the LADDER of 4-component planes (no reference counterpart): the renditions of
// one or several BGRA or RGBA planes of one size as planes of up to eight sizes, every rung in one launch per route.  The bytes are
// chv_scale_lanczos's on one 4-component plane (section 4.4) and the row code is lanczos_rgb_body.hip.h's; the construction is the other
// ladder units': one grid, the concatenation of the rungs' block ranges, largest first; a scalar scan finds the rung.
//
//   lanczos_rgb_ladder<T>     the rungs that take the wave-per-strip route: one WAVE per block of 64 output columns x `rows` output rows of
//                             one picture of one rung.  T: 12 when no strip rung of the launch has more than 12 taps on an axis (four waves
//                             per SIMD), else 22 (three).  <12> holds the strip bodies of 6, 8 and 12 taps, <22> those of 16 and 22 as
//                             well; a rung runs the smallest body over its larger tap count.  A rung's tap counts need not equal its
//                             body's, nor each other.
//   lanczos_rgb_ladder_tile   the rungs that take the tile route: 256-thread blocks, one per 32 x 4 or 8 x 4 output pixels.
#include "lanczos_rgb_body.hip.h"
#include "lanczos_rgb_ladder.h"
#include "lanczos_ladder_launch.hip.h"

namespace chv {

struct RgbRung {
    RgbGeom g;
    int32_t first_block;              // where the rung's range starts in the grid
    int32_t total, per_picture;       // blocks of all pictures, blocks per picture
    int32_t strips;                   // strip route: strips across; tile route: tiles across
    int32_t dst_at;                   // the rung's target within a picture's record
    int32_t pad[3];
};

// (the access rules of the other ladders' arguments: read through the scalar unit from the kernel-argument segment at a uniform index, never
// from a private copy)
struct RgbLadderArgs {
    const DPlane *batch;              // per picture: n_rungs target planes, then the source plane
    int32_t per_image, src_at;        // planes of a picture's record; the source within it
    int32_t rows, pad;                // strip route: output rows per wave (one count for the launch)
    int32_t first[kLanczosPlanarLadderMaxRungs];       // first_block of rung k of this launch (INT_MAX beyond the last): what the scan reads
    RgbRung rung[kLanczosPlanarLadderMaxRungs];
};
static_assert(sizeof(RgbLadderArgs) <= 4096 - 256, "kernel arguments: 4 KB in all, 256 bytes of them the runtime's");

struct RgbBlock {
    RgbGeom g;
    DPlane dst, src;
    int bx, by;
    bool live;
};

// (rung, picture, row chunk / tile row, strip / tile) of block blk of the grid; dst / src from the descriptor list (scalar loads).  XCD: the
// XCD-aware numbering of lanczos3_strip<T> inside the rung's own range, which starts on a multiple of 8 and is padded to one.
template <bool XCD>
CHV_DEV RgbBlock rgb_decode(const RgbLadderArgs &a, int blk) {
    const uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const int r = ladder_rung_of(a.first, blk);
    const RgbRung R = cld<RgbRung>(ka + offsetof(RgbLadderArgs, rung) + (uint64_t)r * sizeof(RgbRung));
    RgbBlock o;
    const LadderItem it = ladder_item<XCD>(blk - R.first_block, R.total);
    o.live = it.live;
    if (!o.live) return o;
    const int picture = it.idx / R.per_picture, rem = it.idx - picture * R.per_picture;
    o.by = rem / R.strips;
    o.bx = rem - o.by * R.strips;
    o.g = R.g;
    const uint64_t rec = (uint64_t)(uintptr_t)a.batch + (uint64_t)picture * a.per_image * sizeof(DPlane);
    o.dst = cld<DPlane>(rec + (uint64_t)R.dst_at * sizeof(DPlane));
    o.src = cld<DPlane>(rec + (uint64_t)a.src_at * sizeof(DPlane));
    return o;
}

// <12> like lanczos3_strip<12> at four waves per SIMD; <22>'s 88 window registers, 22 weights and 22 taps do not fit 128: three
template <int T>
__global__ __launch_bounds__(64, (T <= 12 ? 4 : 3)) void lanczos_rgb_ladder(const RgbLadderArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rgb_ladder_lsm[];
    const RgbBlock blk = rgb_decode<true>(a, blockIdx.x);
    if (!blk.live) return;
#define CHV_RL_CASE(TT) case TT: if constexpr (TT <= T) rgb_strip<TT>(blk.g, blk.dst, blk.src, blk.bx, blk.by, a.rows, rgb_ladder_lsm); break
    switch (blk.g.T) {                // (uniform)
    CHV_RL_CASE(6); CHV_RL_CASE(8); CHV_RL_CASE(12); CHV_RL_CASE(16); CHV_RL_CASE(22);
    default: break;
    }
#undef CHV_RL_CASE
}

__global__ __launch_bounds__(256) void lanczos_rgb_ladder_tile(const RgbLadderArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rgb_ladder_lsm[];
    const RgbBlock blk = rgb_decode<false>(a, blockIdx.x);
    if (!blk.live) return;
    rgb_tile(blk.g, blk.dst, blk.src, blk.bx, blk.by, rgb_ladder_lsm);
}

static hipError_t launch_lanczos_rgb_ladder(const LanczosRgbLadderJob &job, hipStream_t stream, int *launches) {
    *launches = 0;
    if (job.n_pictures < 1 || job.n_rungs < 1 || job.n_rungs > kLanczosPlanarLadderMaxRungs || !job.batch || job.src_w < 1 || job.src_h < 1)
        return hipErrorInvalidValue;
    // every rung's route and numbers before anything is launched: one refused rung refuses the ladder
    RgbRung strip[kLanczosPlanarLadderMaxRungs], tile[kLanczosPlanarLadderMaxRungs];
    int strip_h[kLanczosPlanarLadderMaxRungs], strip_w[kLanczosPlanarLadderMaxRungs];
    int n_strip = 0, n_tile = 0, tmax = 0;
    size_t tile_lds = 0;
    long work = 0;
    for (int r = 0; r < job.n_rungs; r++) {
        const LanczosRgbLadderRung &j = job.rung[r];
        const LanczosPlaneTables &t = j.tab;
        if (j.w < 1 || j.h < 1 || t.tx < 1 || t.ty < 1 || lanczos_refuses(j.w, j.h, job.src_w, job.src_h, t.tx, t.ty)) return hipErrorInvalidValue;
        RgbRung R{};
        R.g.fx = t.fx; R.g.wx = t.wx; R.g.fy = t.fy; R.g.wy = t.wy; R.g.tx = t.tx; R.g.ty = t.ty;
        R.dst_at = r;
        if (rgb_strip_route(j.w, job.src_w, t.tx, t.ty)) {
            R.strips = (j.w + 63) / 64;
            work += (long)R.strips * j.h * job.n_pictures;
            R.g.T = lanczos_tap_class(std::max(t.tx, t.ty));
            tmax = std::max(tmax, R.g.T);
            strip_w[n_strip] = j.w; strip_h[n_strip] = j.h;
            strip[n_strip++] = R;
        } else {
            size_t lds = 0;
            rgb_tile_dims(j.h, job.src_h, t.ty, &R.g.max_rows, &R.g.tw, &lds);
            R.strips = (j.w + R.g.tw - 1) / R.g.tw;
            R.per_picture = R.strips * ((j.h + RT_H - 1) / RT_H);
            const long total = (long)R.per_picture * job.n_pictures;
            if (total > 0x3fffffff || lds > 64 * 1024) return hipErrorInvalidValue;
            R.total = (int32_t)total;
            tile_lds = std::max(tile_lds, lds);
            tile[n_tile++] = R;
        }
    }
    // one count of rows per wave for the launch: the strip rungs share the chip.  A rung's ring is sized for its body's T.
    const int rows = lanczos_strip_rows(work, RS_MAX_ROWS);
    size_t strip_lds = 0;
    for (int k = 0; k < n_strip; k++) {
        RgbRung &R = strip[k];
        R.g.nv = rgb_row_vectors(strip_w[k], job.src_w, R.g.T);
        if (R.g.nv > 64) return hipErrorInvalidValue;              // (cannot happen: a row of tx <= T taps that fits 64 vectors at its ratio fits them with T)
        R.per_picture = R.strips * ((strip_h[k] + rows - 1) / rows);
        const long total = (long)R.per_picture * job.n_pictures;
        if (total > 0x3fffffff) return hipErrorInvalidValue;
        R.total = (int32_t)total;
        strip_lds = std::max(strip_lds, lanczos_wtab_bytes(rows, R.g.T) + (size_t)2 * R.g.nv * 16);
    }
    RgbLadderArgs a{};
    a.batch = job.batch; a.per_image = job.n_rungs + 1; a.src_at = job.n_rungs; a.rows = rows;
    RgbLadderArgs t = a;
    unsigned strip_grid = 0, tile_grid = 0;
    if (n_strip && !ladder_order(&a, strip, n_strip, 8, &strip_grid)) return hipErrorInvalidValue;
    if (n_tile && !ladder_order(&t, tile, n_tile, 1, &tile_grid)) return hipErrorInvalidValue;
    return ladder_launch(launches, n_strip, [&] {
        if (tmax <= 12) hipLaunchKernelGGL(lanczos_rgb_ladder<12>, dim3(strip_grid), dim3(64), strip_lds, stream, a);
        else hipLaunchKernelGGL(lanczos_rgb_ladder<22>, dim3(strip_grid), dim3(64), strip_lds, stream, a);
    }, n_tile, [&] { hipLaunchKernelGGL(lanczos_rgb_ladder_tile, dim3(tile_grid), dim3(256), tile_lds, stream, t); });
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosRgbLadderRegistrar {
    LanczosRgbLadderRegistrar() { register_lanczos_rgb_ladder_launcher(launch_lanczos_rgb_ladder); }
} g_lanczos_rgb_ladder_registrar;

}  // namespace chv
