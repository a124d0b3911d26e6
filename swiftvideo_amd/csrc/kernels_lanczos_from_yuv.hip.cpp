// kernels_lanczos_from_yuv.hip.cpp — Lanczos-3 resize of an NV12 or y420p picture straight into a BGRA / RGBA plane (DESIGN.md section 4.4.6;
// no reference counterpart): the logical planes Y, Cb and Cr each go through the 1-component chain of chv_scale_lanczos to the TARGET's size
// (the chroma planes straight from cw x ch), are rounded to codes, and a pixel's three codes go through the integer matrix of section 4.2.
// ONE launch covers every picture of a batch chunk; a lone call's planes travel in the kernel arguments, a batch's through the descriptor ring.
//
//   lanczos_from_yuv_strip<MAXT, SC>   no plane has more than 22 taps on an axis: one WAVE per block of 64 output columns x `rows` output rows
//                                      of one picture.  It resamples Cb, then Cr, for the block (fy_strip with the chroma tables; SC = 2 reads
//                                      the CbCr plane of NV12 at a tap stride of two, SC = 1 the planes of y420p) and leaves the CODES in
//                                      LDS, 2 x 64 x rows bytes; then it runs the luma strip over the same block, and a finished luma row
//                                      takes the lane's two codes back, applies the matrix and stores one dword per lane.  MAXT = 12 holds
//                                      the luma bodies of 6, 8 and 12 taps, MAXT = 22 those of 16 and 22; both hold the chroma bodies of 6, 8
//                                      and 12 (chroma never has more on this route: fy_strip_route).
//   lanczos_from_yuv_tile              everything else, both packings: 256-thread blocks, one per 32 x 4 output pixels; the three planes take
//                                      turns in one LDS array.  Simple on purpose.
#include "lanczos_from_yuv_body.hip.h"
#include "lanczos_from_yuv.h"

namespace chv {

struct FyTab {
    const int32_t *fx; const float *wx;
    const int32_t *fy; const float *wy;
    int32_t tx, ty;
    int32_t nv, T;                    // strip route: vectors of one staged row, the body's tap class
    int32_t max_rows, pad;            // tile route: rows of the LDS array
};

struct FromYuvArgs {
    const DPlane *batch;              // per picture: the target, then the source's planes; null: the planes below
    DPlane dst, y, c0, c1;            // c0: CbCr (NV12) or Cb (y420p); c1: Cr (y420p), c0 again for NV12
    FyTab luma, chroma;
    int32_t src_planes, rgba;
    int32_t rows, codes_at;           // strip route: output rows per wave, where the codes start in the wave's LDS
    int32_t strips, chunks, per_picture, total;
    Csc k;
};

// The block's planes and tables are read where a phase needs them, through the scalar unit, from the kernel arguments (or the picture's record
// of the descriptor list) behind a pointer the compiler cannot see through: what the luma phase needs does not sit in registers while the
// chroma phases run.
CHV_DEV uint64_t fy_opaque(uint64_t v) { asm volatile("" : "+s"(v) :: "memory"); return v; }

// the record of picture `picture` in the descriptor list, 0 for a lone call (uniform)
CHV_DEV uint64_t fy_record(uint64_t ka, int picture, int src_planes) {
    const uint64_t batch = cld<uint64_t>(ka + offsetof(FromYuvArgs, batch));
    return batch ? batch + (uint64_t)picture * (1 + src_planes) * sizeof(DPlane) : 0;
}

// plane `which` of the block's picture: 0 the target, 1 Y, 2 CbCr / Cb, 3 Cr (NV12: the CbCr plane again).  rec: the picture's record, or 0
CHV_DEV DPlane fy_block_plane(uint64_t ka, uint64_t rec, int which, int src_planes) {
    const uint64_t addr = rec ? rec + (uint64_t)min(which, src_planes) * sizeof(DPlane)
                              : ka + offsetof(FromYuvArgs, dst) + (uint64_t)which * sizeof(DPlane);
    return cld<DPlane>(addr);
}

// a logical plane as the shared bodies see one: the target's size with one component, the plane that holds it
CHV_DEV PlanarPlane fy_plane(const FyTab &t, int ow, int oh, const DPlane &src) {
    PlanarPlane g;
    g.fx = t.fx; g.wx = t.wx; g.fy = t.fy; g.wy = t.wy;
    g.dst = DPlane{ nullptr, ow, oh, 0, 1 };
    g.src = src;
    g.tx = t.tx; g.ty = t.ty; g.strips = 0; g.chunks = 0; g.nv = t.nv; g.max_rows = t.max_rows; g.first = 0; g.pad = 0;
    return g;
}

template <int MAXT, int SC>
__global__ __launch_bounds__(64, 4) void lanczos_from_yuv_strip(const FromYuvArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fy_lsm[];
    const int b = blockIdx.x, per_xcd = (a.total + 7) >> 3;       // XCD-aware numbering, as in lanczos_yuv_strip<T>
    const int idx = (b & 7) * per_xcd + (b >> 3);
    if ((b >> 3) >= per_xcd || idx >= a.total) return;
    const int picture = idx / a.per_picture, rem = idx - picture * a.per_picture;
    const int chunk = rem / a.strips, strip = rem - chunk * a.strips;
    const int lane = threadIdx.x, rows = a.rows;
    constexpr int src_planes = SC == 2 ? 2 : 3;                   // (the tap stride of chroma says which packing this is)
    uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    uint8_t *codes = fy_lsm + a.codes_at + lane;                  // [2][rows][64]: this lane's column of them
    // Cb, then Cr: the codes of the block, to LDS
#pragma nounroll
    for (int c = 0; c < 2; c++) {
        ka = fy_opaque(ka);
        const uint64_t rec = fy_record(ka, picture, src_planes);
        const int ow = cld<int32_t>(ka + offsetof(FromYuvArgs, dst) + offsetof(DPlane, w)), oh = cld<int32_t>(ka + offsetof(FromYuvArgs, dst) + offsetof(DPlane, h));
        const FyTab t = cld<FyTab>(ka + offsetof(FromYuvArgs, chroma));
        const PlanarPlane g = fy_plane(t, ow, oh, fy_block_plane(ka, rec, SC == 1 ? 2 + c : 2, src_planes));
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
    ka = fy_opaque(ka);
    const uint64_t rec = fy_record(ka, picture, src_planes);
    const int ow = cld<int32_t>(ka + offsetof(FromYuvArgs, dst) + offsetof(DPlane, w)), oh = cld<int32_t>(ka + offsetof(FromYuvArgs, dst) + offsetof(DPlane, h));
    const FyTab t = cld<FyTab>(ka + offsetof(FromYuvArgs, luma));
    const PlanarPlane g = fy_plane(t, ow, oh, fy_block_plane(ka, rec, 1, src_planes));
    const DPlane dst = fy_block_plane(ka, rec, 0, src_planes);
    const Csc k = cld<Csc>(ka + offsetof(FromYuvArgs, k));
    const bool rgba = cld<int32_t>(ka + offsetof(FromYuvArgs, rgba)) != 0;
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
    case 6: if constexpr (MAXT <= 12) fy_strip<6, 1>(g, 0, strip, chunk, rows, fy_lsm, sink); break;
    case 8: if constexpr (MAXT <= 12) fy_strip<8, 1>(g, 0, strip, chunk, rows, fy_lsm, sink); break;
    case 12: if constexpr (MAXT <= 12) fy_strip<12, 1>(g, 0, strip, chunk, rows, fy_lsm, sink); break;
    case 16: if constexpr (MAXT > 12) fy_strip<16, 1>(g, 0, strip, chunk, rows, fy_lsm, sink); break;
    case 22: if constexpr (MAXT > 12) fy_strip<22, 1>(g, 0, strip, chunk, rows, fy_lsm, sink); break;
    default: break;
    }
}

__global__ __launch_bounds__(256) void lanczos_from_yuv_tile(const FromYuvArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fy_lsm[];
    const int idx = blockIdx.x;
    if (idx >= a.total) return;
    const int picture = idx / a.per_picture, rem = idx - picture * a.per_picture;
    const int by = rem / a.strips, bx = rem - by * a.strips;
    const int ow = a.dst.w, oh = a.dst.h, src_planes = a.src_planes;
    const uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const uint64_t rec = fy_record(ka, picture, src_planes);
    const bool nv12 = src_planes == 2;
    const DPlane c0 = fy_block_plane(ka, rec, 2, src_planes), c1 = fy_block_plane(ka, rec, 3, src_planes);
    const DPlane yp = fy_block_plane(ka, rec, 1, src_planes), dst = fy_block_plane(ka, rec, 0, src_planes);
    const PlanarPlane gc = fy_plane(a.chroma, ow, oh, c0), gl = fy_plane(a.luma, ow, oh, yp);
    const uint32_t u = fy_tile_plane(gc, c0.ptr, c0.pitch, nv12 ? 2 : 1, bx, by, fy_lsm);
    const uint32_t v = fy_tile_plane(gc, nv12 ? c0.ptr + 1 : c1.ptr, nv12 ? c0.pitch : c1.pitch, nv12 ? 2 : 1, bx, by, fy_lsm);
    const uint32_t y = fy_tile_plane(gl, yp.ptr, yp.pitch, 1, bx, by, fy_lsm);
    const int tid = threadIdx.x;
    const int x = bx * PT_W + tid % PT_W, oy = by * PT_H + tid / PT_W;
    if (tid < PT_W * PT_H && x < ow && oy < oh)
        gst<uint32_t>(dst.ptr + (size_t)oy * dst.pitch + (size_t)x * 4, fy_pixel(a.k, a.rgba != 0, (int)y, (int)u, (int)v));
}

static hipError_t launch_lanczos_from_yuv(const LanczosFromYuvJob &job, hipStream_t stream) {
    if ((job.src_planes != 2 && job.src_planes != 3) || job.n_pictures < 1) return hipErrorInvalidValue;
    const bool nv12 = job.src_planes == 2;
    const DPlane &d = job.dst;
    // the logical planes luma and chroma (Cb and Cr have one size); one refused plane refuses the picture, and nothing is launched
    PlanarPlane pl[2]{};
    for (int p = 0; p < 2; p++) {
        const LanczosPlaneTables &t = p ? job.chroma : job.luma;
        PlanarPlane &g = pl[p];
        g.fx = t.fx; g.wx = t.wx; g.fy = t.fy; g.wy = t.wy; g.tx = t.tx; g.ty = t.ty;
        g.dst = DPlane{ nullptr, d.w, d.h, 0, 1 };
        g.src = DPlane{ nullptr, job.src[p].w, job.src[p].h, 0, p && nv12 ? 2 : 1 };
        if (g.dst.w < 1 || g.dst.h < 1 || g.src.w < 1 || g.src.h < 1 || lanczos_refuses(g.dst.w, g.dst.h, g.src.w, g.src.h, t.tx, t.ty)) return hipErrorInvalidValue;
    }
    FromYuvArgs a{};
    a.batch = job.batch;
    a.dst = d; a.y = job.src[0]; a.c0 = job.src[1]; a.c1 = job.src[nv12 ? 1 : 2];
    a.src_planes = job.src_planes; a.rgba = job.rgba;
    a.k = Csc{ job.yoff, job.cy, job.crv, job.cgu, job.cgv, job.cbu };
    auto tab = [](const PlanarPlane &g, int T) { return FyTab{ g.fx, g.wx, g.fy, g.wy, g.tx, g.ty, g.nv, T, g.max_rows, 0 }; };
    (void)hipGetLastError();
    int TL = 0, TC = 0, ring = 0;
    if (fy_strip_route(pl, &TL, &TC, &ring)) {
        a.strips = (d.w + 63) / 64;
        a.rows = fy_strip_rows((long)a.strips * d.h * job.n_pictures);
        a.chunks = (d.h + a.rows - 1) / a.rows;
        a.per_picture = a.strips * a.chunks;
        const long total = (long)a.per_picture * job.n_pictures;
        if (total > 0x3fffffff) return hipErrorInvalidValue;
        a.total = (int32_t)total;
        a.codes_at = (int32_t)fy_codes_at(a.rows, TL, TC, ring);
        a.luma = tab(pl[0], TL); a.chroma = tab(pl[1], TC);
        const dim3 grid((unsigned)(((a.total + 7) / 8) * 8));
        const size_t lds = fy_strip_lds(a.rows, TL, TC, ring);
        if (TL <= 12) {
            if (nv12) hipLaunchKernelGGL((lanczos_from_yuv_strip<12, 2>), grid, dim3(64), lds, stream, a);
            else hipLaunchKernelGGL((lanczos_from_yuv_strip<12, 1>), grid, dim3(64), lds, stream, a);
        } else {
            if (nv12) hipLaunchKernelGGL((lanczos_from_yuv_strip<22, 2>), grid, dim3(64), lds, stream, a);
            else hipLaunchKernelGGL((lanczos_from_yuv_strip<22, 1>), grid, dim3(64), lds, stream, a);
        }
        return hipGetLastError();
    }
    int rows_max = 0;
    a.per_picture = planar_tile_blocks(pl, 2, &rows_max) / 2;     // (both records count the target's tiles)
    a.strips = pl[0].strips; a.chunks = pl[0].chunks;
    const long total = (long)a.per_picture * job.n_pictures;
    const size_t lds = (size_t)rows_max * PT_W * sizeof(float);
    if (total > 0x3fffffff || lds > 64 * 1024) return hipErrorInvalidValue;
    a.total = (int32_t)total;
    a.luma = tab(pl[0], 0); a.chroma = tab(pl[1], 0);
    hipLaunchKernelGGL(lanczos_from_yuv_tile, dim3((unsigned)a.total), dim3(256), lds, stream, a);
    return hipGetLastError();
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosFromYuvRegistrar { LanczosFromYuvRegistrar() { register_lanczos_from_yuv_launcher(launch_lanczos_from_yuv); } } g_lanczos_from_yuv_registrar;

}  // namespace chv
