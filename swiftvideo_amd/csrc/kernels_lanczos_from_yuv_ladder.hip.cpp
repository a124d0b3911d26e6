// kernels_lanczos_from_yuv_ladder.hip.cpp — the decoder side's LADDER (no reference counterpart): the renditions of
// one or several NV12 or y420p pictures of one size as BGRA / RGBA planes of up to eight sizes, every rung in one launch per route.  The bytes
// are chv_scale_lanczos_from_yuv's (section 4.4.6) and the row code is lanczos_from_yuv_body.hip.h's, unchanged; the construction is
// kernels_lanczos_420.hip.cpp's: one grid, the concatenation of the rungs' block ranges, largest first; a scalar scan finds the rung.
//
//   lanczos_from_yuv_ladder<MAXT, SC>   the rungs that take the wave-per-strip route: one WAVE per block of 64 output columns x `rows` output
//                                       rows of one picture of one rung, lanczos_from_yuv_strip's three passes (Cb, Cr to codes in LDS, then
//                                       luma and the pixel).  MAXT: the largest luma tap class among the launch's strip rungs — <12, .> holds
//                                       the luma bodies of 6, 8 and 12 taps, <22, .> those of 16 and 22 as well; both hold the chroma bodies
//                                       of 6, 8 and 12.  SC = 2 reads the CbCr plane of NV12, SC = 1 the planes of y420p.
//   lanczos_from_yuv_ladder_tile        the rungs that take the tile route, both packings: 256-thread blocks, one per 32 x 4 output pixels.
#include "lanczos_from_yuv_body.hip.h"
#include "lanczos_from_yuv_ladder.h"
#include "lanczos_ladder_launch.hip.h"

namespace chv {

// (kernels_lanczos_from_yuv.hip.cpp's record, member by member)
struct FyTab {
    const int32_t *fx; const float *wx;
    const int32_t *fy; const float *wy;
    int32_t tx, ty;
    int32_t nv, T;                    // strip route: vectors of one staged row, the body's tap class
    int32_t max_rows, pad;            // tile route: rows of the LDS array
};

struct FylRung {
    int32_t first_block;              // where the rung's range starts in the grid
    int32_t total, per_picture;       // blocks of all pictures, blocks per picture
    int32_t strips, chunks;           // strip route: strips across, row chunks down; tile route: tiles across and down
    int32_t rows, codes_at;           // strip route: output rows per wave, where the codes start in the wave's LDS
    int32_t w, h;                     // the rung's target size
    int32_t dst_at;                   // the rung's target within a picture's record
    int32_t pad[2];
    FyTab luma, chroma;
};

// (the access rules of X420Args and FromYuvArgs: read through the scalar unit from the kernel-argument segment at a uniform index, never
// from a private copy; what the luma pass needs is loaded when the luma pass begins, behind the laundered pointer)
struct FylArgs {
    const DPlane *batch;              // per picture: n_rungs target planes, then the source's planes
    Csc k;
    int32_t rgba, src_planes;
    int32_t per_image, src_at;        // planes of a picture's record; the source's first plane within it
    int32_t first[kLanczosPlanarLadderMaxRungs];
    FylRung rung[kLanczosPlanarLadderMaxRungs];
};
static_assert(sizeof(FylArgs) <= 4096 - 256, "kernel arguments: 4 KB in all, 256 bytes of them the runtime's");

CHV_DEV uint64_t fyl_opaque(uint64_t v) { asm volatile("" : "+s"(v) :: "memory"); return v; }

// rung r's record in the kernel-argument segment; the record of picture `picture` in the descriptor list (both uniform)
CHV_DEV uint64_t fyl_rung(uint64_t ka, int r) { return ka + offsetof(FylArgs, rung) + (uint64_t)r * sizeof(FylRung); }
CHV_DEV uint64_t fyl_record(uint64_t ka, int picture) {
    return cld<uint64_t>(ka + offsetof(FylArgs, batch)) + (uint64_t)picture * cld<int32_t>(ka + offsetof(FylArgs, per_image)) * sizeof(DPlane);
}
// source plane `which` of the picture: 0 Y, 1 CbCr / Cb, 2 Cr
CHV_DEV DPlane fyl_src_plane(uint64_t ka, uint64_t rec, int which) {
    return cld<DPlane>(rec + (uint64_t)(cld<int32_t>(ka + offsetof(FylArgs, src_at)) + which) * sizeof(DPlane));
}

CHV_DEV PlanarPlane fyl_plane(const FyTab &t, int ow, int oh, const DPlane &src) {
    PlanarPlane g;
    g.fx = t.fx; g.wx = t.wx; g.fy = t.fy; g.wy = t.wy;
    g.dst = DPlane{ nullptr, ow, oh, 0, 1 };
    g.src = src;
    g.tx = t.tx; g.ty = t.ty; g.strips = 0; g.chunks = 0; g.nv = t.nv; g.max_rows = t.max_rows; g.first = 0; g.pad = 0;
    return g;
}

template <int MAXT, int SC>
__global__ __launch_bounds__(64, 4) void lanczos_from_yuv_ladder(const FylArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fy_lsm[];
    const int r = ladder_rung_of(a.first, blockIdx.x);
    uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    int picture, chunk, strip, codes_at;
    {
        const uint64_t R = fyl_rung(ka, r);
        const int b = (int)blockIdx.x - cld<int32_t>(R + offsetof(FylRung, first_block));
        const int total = cld<int32_t>(R + offsetof(FylRung, total)), per_picture = cld<int32_t>(R + offsetof(FylRung, per_picture));
        const int strips = cld<int32_t>(R + offsetof(FylRung, strips));
        const LadderItem it = ladder_item<true>(b, total);        // XCD-aware numbering inside the rung's own (padded) range
        if (!it.live) return;
        picture = it.idx / per_picture;
        const int rem = it.idx - picture * per_picture;
        chunk = rem / strips; strip = rem - chunk * strips;
        codes_at = cld<int32_t>(R + offsetof(FylRung, codes_at));
    }
    const int lane = threadIdx.x;
    uint8_t *codes = fy_lsm + codes_at + lane;                    // [2][rows][64]: this lane's column of them
    // Cb, then Cr: the codes of the block, to LDS
#pragma nounroll
    for (int c = 0; c < 2; c++) {
        ka = fyl_opaque(ka);
        const uint64_t R = fyl_rung(ka, r), rec = fyl_record(ka, picture);
        const int ow = cld<int32_t>(R + offsetof(FylRung, w)), oh = cld<int32_t>(R + offsetof(FylRung, h)), rows = cld<int32_t>(R + offsetof(FylRung, rows));
        const FyTab t = cld<FyTab>(R + offsetof(FylRung, chroma));
        const PlanarPlane g = fyl_plane(t, ow, oh, fyl_src_plane(ka, rec, SC == 1 ? 1 + c : 1));
        uint8_t *out = codes + c * rows * 64;
        auto sink = [&](int j, float o) { out[j * 64] = (uint8_t)to_code_raw(o); };
        const int comp = SC == 2 ? c : 0;
        switch (t.T) {                // (uniform)
        case 6: fy_strip<6, SC>(g, comp, strip, chunk, rows, fy_lsm, sink); break;
        case 8: fy_strip<8, SC>(g, comp, strip, chunk, rows, fy_lsm, sink); break;
        default: fy_strip<12, SC>(g, comp, strip, chunk, rows, fy_lsm, sink); break;
        }
    }
    // luma, and the pixel: a lane reads the two codes it wrote itself
    ka = fyl_opaque(ka);
    const uint64_t R = fyl_rung(ka, r), rec = fyl_record(ka, picture);
    const int ow = cld<int32_t>(R + offsetof(FylRung, w)), oh = cld<int32_t>(R + offsetof(FylRung, h)), rows = cld<int32_t>(R + offsetof(FylRung, rows));
    const FyTab t = cld<FyTab>(R + offsetof(FylRung, luma));
    const PlanarPlane g = fyl_plane(t, ow, oh, fyl_src_plane(ka, rec, 0));
    const DPlane dst = cld<DPlane>(rec + (uint64_t)cld<int32_t>(R + offsetof(FylRung, dst_at)) * sizeof(DPlane));
    const Csc k = cld<Csc>(ka + offsetof(FylArgs, k));
    const bool rgba = cld<int32_t>(ka + offsetof(FylArgs, rgba)) != 0;
    const int x = strip * 64 + lane;
    const bool inside = x < ow;
    uint8_t *px = dst.ptr + (size_t)chunk * rows * dst.pitch + (size_t)x * 4;
    const uint8_t *cb = codes, *cr = codes + rows * 64;
    const int pitch = dst.pitch;
    auto sink = [&](int j, float o) {
        const uint32_t w = fy_pixel(k, rgba, (int)to_code_raw(o), (int)cb[j * 64], (int)cr[j * 64]);
        if (inside) gst<uint32_t>(px + (size_t)j * pitch, w);
    };
    switch (t.T) {                    // (uniform)
    case 6: fy_strip<6, 1>(g, 0, strip, chunk, rows, fy_lsm, sink); break;
    case 8: fy_strip<8, 1>(g, 0, strip, chunk, rows, fy_lsm, sink); break;
    case 12: fy_strip<12, 1>(g, 0, strip, chunk, rows, fy_lsm, sink); break;
    case 16: if constexpr (MAXT > 12) fy_strip<16, 1>(g, 0, strip, chunk, rows, fy_lsm, sink); break;
    case 22: if constexpr (MAXT > 12) fy_strip<22, 1>(g, 0, strip, chunk, rows, fy_lsm, sink); break;
    default: break;
    }
}

__global__ __launch_bounds__(256) void lanczos_from_yuv_ladder_tile(const FylArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fy_lsm[];
    const int r = ladder_rung_of(a.first, blockIdx.x);
    const uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const uint64_t R = fyl_rung(ka, r);
    const int idx = (int)blockIdx.x - cld<int32_t>(R + offsetof(FylRung, first_block));
    if (idx >= cld<int32_t>(R + offsetof(FylRung, total))) return;
    const int per_picture = cld<int32_t>(R + offsetof(FylRung, per_picture)), strips = cld<int32_t>(R + offsetof(FylRung, strips));
    const int picture = idx / per_picture, rem = idx - picture * per_picture;
    const int by = rem / strips, bx = rem - by * strips;
    const int ow = cld<int32_t>(R + offsetof(FylRung, w)), oh = cld<int32_t>(R + offsetof(FylRung, h));
    const bool nv12 = a.src_planes == 2;
    const uint64_t rec = fyl_record(ka, picture);
    const DPlane c0 = fyl_src_plane(ka, rec, 1), c1 = fyl_src_plane(ka, rec, nv12 ? 1 : 2);
    const DPlane yp = fyl_src_plane(ka, rec, 0);
    const DPlane dst = cld<DPlane>(rec + (uint64_t)cld<int32_t>(R + offsetof(FylRung, dst_at)) * sizeof(DPlane));
    const PlanarPlane gc = fyl_plane(cld<FyTab>(R + offsetof(FylRung, chroma)), ow, oh, c0);
    const PlanarPlane gl = fyl_plane(cld<FyTab>(R + offsetof(FylRung, luma)), ow, oh, yp);
    const uint32_t u = fy_tile_plane(gc, c0.ptr, c0.pitch, nv12 ? 2 : 1, bx, by, fy_lsm);
    const uint32_t v = fy_tile_plane(gc, nv12 ? c0.ptr + 1 : c1.ptr, nv12 ? c0.pitch : c1.pitch, nv12 ? 2 : 1, bx, by, fy_lsm);
    const uint32_t y = fy_tile_plane(gl, yp.ptr, yp.pitch, 1, bx, by, fy_lsm);
    const int tid = threadIdx.x;
    const int x = bx * PT_W + tid % PT_W, oy = by * PT_H + tid / PT_W;
    if (tid < PT_W * PT_H && x < ow && oy < oh)
        gst<uint32_t>(dst.ptr + (size_t)oy * dst.pitch + (size_t)x * 4, fy_pixel(a.k, a.rgba != 0, (int)y, (int)u, (int)v));
}

// one rung of one route, before the launch's order is known
struct FylPending {
    FylRung R;
    int TL, TC, ring;                 // strip route: the tap classes of luma and chroma, the longest ring slot
    long work;                        // strip route: the (strip, output row) pairs of all pictures
};

static hipError_t launch_lanczos_from_yuv_ladder(const LanczosFromYuvLadderJob &job, hipStream_t stream, int *launches) {
    *launches = 0;
    if ((job.src_planes != 2 && job.src_planes != 3) || job.n_pictures < 1 || job.n_rungs < 1 || job.n_rungs > kLanczosPlanarLadderMaxRungs ||
        !job.batch)
        return hipErrorInvalidValue;
    const bool nv12 = job.src_planes == 2;
    auto tab = [](const PlanarPlane &g, int T) { return FyTab{ g.fx, g.wx, g.fy, g.wy, g.tx, g.ty, g.nv, T, g.max_rows, 0 }; };
    // every rung's route and numbers before anything is launched: one refused rung refuses the ladder
    FylPending strip[kLanczosPlanarLadderMaxRungs], tile[kLanczosPlanarLadderMaxRungs];
    int n_strip = 0, n_tile = 0, max_tl = 0;
    size_t tile_lds = 0;
    long work = 0;
    for (int r = 0; r < job.n_rungs; r++) {
        const LanczosFromYuvLadderRung &j = job.rung[r];
        // the logical planes luma and chroma (Cb and Cr have one size) of this rung, as the single call sees them
        PlanarPlane pl[2]{};
        for (int p = 0; p < 2; p++) {
            const LanczosPlaneTables &t = p ? j.chroma : j.luma;
            PlanarPlane &g = pl[p];
            g.fx = t.fx; g.wx = t.wx; g.fy = t.fy; g.wy = t.wy; g.tx = t.tx; g.ty = t.ty;
            g.dst = DPlane{ nullptr, j.w, j.h, 0, 1 };
            g.src = DPlane{ nullptr, p ? job.chroma_w : job.luma_w, p ? job.chroma_h : job.luma_h, 0, p && nv12 ? 2 : 1 };
            if (g.dst.w < 1 || g.dst.h < 1 || g.src.w < 1 || g.src.h < 1 || lanczos_refuses(g.dst.w, g.dst.h, g.src.w, g.src.h, t.tx, t.ty)) return hipErrorInvalidValue;
        }
        FylPending P{};
        P.R.w = j.w; P.R.h = j.h; P.R.dst_at = r;
        if (fy_strip_route(pl, &P.TL, &P.TC, &P.ring)) {          // (the route its single call takes)
            P.R.strips = (j.w + 63) / 64;
            P.work = (long)P.R.strips * j.h * job.n_pictures;
            work += P.work;
            max_tl = std::max(max_tl, P.TL);
            P.R.luma = tab(pl[0], P.TL); P.R.chroma = tab(pl[1], P.TC);
            strip[n_strip++] = P;
        } else {
            int rows_max = 0;
            P.R.per_picture = planar_tile_blocks(pl, 2, &rows_max) / 2;       // (both records count the target's tiles)
            P.R.strips = pl[0].strips; P.R.chunks = pl[0].chunks;
            const long total = (long)P.R.per_picture * job.n_pictures;
            const size_t lds = (size_t)rows_max * PT_W * sizeof(float);
            if (total > 0x3fffffff || lds > 64 * 1024) return hipErrorInvalidValue;
            P.R.total = (int32_t)total;
            P.R.luma = tab(pl[0], 0); P.R.chroma = tab(pl[1], 0);
            tile_lds = std::max(tile_lds, lds);
            tile[n_tile++] = P;
        }
    }
    // rows per wave from the (strip, output row) pairs of the whole launch: the strip rungs share the chip
    const int rows = fy_strip_rows(work);
    size_t strip_lds = 0;
    for (int k = 0; k < n_strip; k++) {
        FylPending &P = strip[k];
        P.R.rows = rows;
        P.R.chunks = (P.R.h + rows - 1) / rows;
        P.R.per_picture = P.R.strips * P.R.chunks;
        const long total = (long)P.R.per_picture * job.n_pictures;
        if (total > 0x3fffffff) return hipErrorInvalidValue;
        P.R.total = (int32_t)total;
        P.R.codes_at = (int32_t)fy_codes_at(rows, P.TL, P.TC, P.ring);
        strip_lds = std::max(strip_lds, fy_strip_lds(rows, P.TL, P.TC, P.ring));
    }
    FylArgs a{};
    a.batch = job.batch;
    a.k = Csc{ job.yoff, job.cy, job.crv, job.cgu, job.cgv, job.cbu };
    a.rgba = job.rgba; a.src_planes = job.src_planes;
    a.per_image = job.n_rungs + job.src_planes; a.src_at = job.n_rungs;
    FylArgs t = a;
    unsigned strip_grid = 0, tile_grid = 0;
    const auto total = [](const FylPending &P) { return P.R.total; };
    const auto copy = [](FylArgs *to, int k, const FylPending &P) { to->rung[k] = P.R; };
    if (n_strip && !ladder_order(&a, strip, n_strip, 8, &strip_grid, total, copy)) return hipErrorInvalidValue;
    if (n_tile && !ladder_order(&t, tile, n_tile, 1, &tile_grid, total, copy)) return hipErrorInvalidValue;
    return ladder_launch(launches, n_strip, [&] {
        if (max_tl <= 12) {
            if (nv12) hipLaunchKernelGGL((lanczos_from_yuv_ladder<12, 2>), dim3(strip_grid), dim3(64), strip_lds, stream, a);
            else hipLaunchKernelGGL((lanczos_from_yuv_ladder<12, 1>), dim3(strip_grid), dim3(64), strip_lds, stream, a);
        } else {
            if (nv12) hipLaunchKernelGGL((lanczos_from_yuv_ladder<22, 2>), dim3(strip_grid), dim3(64), strip_lds, stream, a);
            else hipLaunchKernelGGL((lanczos_from_yuv_ladder<22, 1>), dim3(strip_grid), dim3(64), strip_lds, stream, a);
        }
    }, n_tile, [&] { hipLaunchKernelGGL(lanczos_from_yuv_ladder_tile, dim3(tile_grid), dim3(256), tile_lds, stream, t); });
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosFromYuvLadderRegistrar {
    LanczosFromYuvLadderRegistrar() { register_lanczos_from_yuv_ladder_launcher(launch_lanczos_from_yuv_ladder); }
} g_lanczos_from_yuv_ladder_registrar;

}  // namespace chv
