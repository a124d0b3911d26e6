// kernels_lanczos_to_yuv.hip.cpp — Lanczos-3 resize of one BGRA / RGBA plane straight into an NV12 or y420p picture (DESIGN.md section 4.4.2;
// no reference counterpart): the three colour channels go through the chain of kernels_lanczos.hip.cpp (horizontal then vertical pass, one
// fused multiply-add per tap from 0.0f, taps ascending, float intermediate, convert_uchar_sat_rte), and the codes — still in registers — through
// the integer matrix of section 4.5: luma per pixel, Cb and Cr from the rounded mean of the 2 x 2 codes a chroma texel covers.  The alpha channel is
// never filtered: three chains per tap where the BGRA -> BGRA kernels run four.
//
// ONE launch covers every picture of a batch chunk.  The matrix arrives in the source's byte order (the host exchanges two columns for BGRA),
// so no kernel asks which byte is red.
//
//   lanczos_yuv_strip<T>  tx == ty == T <= 22, a staged row of at most 64 vectors: one WAVE per strip of 64 output columns x `rows` output rows
//                         (rows even: a chunk starts on an even row), the structure of lanczos3_strip<T>.  A finished row gives the lane's luma —
//                         a quad's four bytes gathered with two quad-permute DPP moves, one dword store — and its packed codes; an even row's
//                         codes wait one row in a register, the odd row adds the pair lane's two rows through DPP and the even lane stores.
//   lanczos_yuv_tile      everything else (unequal or more than 22 taps, long staged rows, sources narrower than a vector): tw x 4 output pixels
//                         per block (tw 32, 8 for large reductions), horizontal pass from global memory into LDS, vertical pass out of it with
//                         a quad of lanes on a 2 x 2 pixel block.  Simple on purpose.
//
// The row code of both lives in lanczos_to_yuv_body.hip.h, shared with the ladder unit (kernels_lanczos_ladder.hip.cpp); the kernels here find
// their block's picture and position and call it.
#include "lanczos_to_yuv_body.hip.h"
#include "lanczos_to_yuv.h"

namespace chv {

// ---------------------------------------------------------------------------------------------------------------------
// lanczos_yuv_strip<T> — one geometry, every picture of a batch chunk: the block's picture, row chunk and strip, then the shared strip body.
template <int T>
__global__ __launch_bounds__(64, (T >= 18 ? 3 : 4)) void lanczos_yuv_strip(const ToYuvArgs a) {
    const int b = blockIdx.x, per_xcd = (a.total + 7) >> 3;       // XCD-aware numbering, as in lanczos3_strip2
    const int idx = (b & 7) * per_xcd + (b >> 3);
    if ((b >> 3) >= per_xcd || idx >= a.total) return;
    const int image = idx / a.per_picture, rem = idx - image * a.per_picture;
    const int chunk = rem / a.strips, strip = rem - chunk * a.strips;
    const ToYuvPlanes P = yuv_planes(a, image);
    lanczos_yuv_strip_body<T>(a, P, a, chunk, strip);
}

// ---------------------------------------------------------------------------------------------------------------------
// lanczos_yuv_tile — any tap counts: the block's picture and tile, then the shared tile body.
__global__ __launch_bounds__(256) void lanczos_yuv_tile(const ToYuvArgs a) {
    const int idx = blockIdx.x;
    if (idx >= a.total) return;
    const int image = idx / a.per_picture, rem = idx - image * a.per_picture;
    const int by = rem / a.strips, bx = rem - by * a.strips;
    const ToYuvPlanes P = yuv_planes(a, image);
    lanczos_yuv_tile_body(a, P, a, by, bx);
}

static hipError_t launch_lanczos_to_yuv(const LanczosToYuvJob &job, hipStream_t stream) {
    if ((job.n_dst != 2 && job.n_dst != 3) || job.n_pictures < 1) return hipErrorInvalidValue;
    const DPlane &d = job.dst[0], &s = job.src;
    if (lanczos_refuses(d.w, d.h, s.w, s.h, job.tx, job.ty)) return hipErrorInvalidValue;          // nothing is launched
    ToYuvArgs a{};
    a.fx = job.fx; a.wx = job.wx; a.fy = job.fy; a.wy = job.wy; a.tx = job.tx; a.ty = job.ty;
    a.y = job.dst[0]; a.c0 = job.dst[1]; a.c1 = job.dst[job.n_dst == 3 ? 2 : 1]; a.src = s;
    a.batch = job.batch; a.n_dst = job.n_dst;
    a.ybase = (job.yoff << 16) + 32768;
    a.ky0 = job.ky[0]; a.ky1 = job.ky[1]; a.ky2 = job.ky[2];
    a.ku0 = job.ku[0]; a.ku1 = job.ku[1]; a.ku2 = job.ku[2];
    a.kv0 = job.kv[0]; a.kv1 = job.kv[1]; a.kv2 = job.kv[2];
    (void)hipGetLastError();
    // equal tap counts on both axes, a staged row of at most 64 vectors: the wave-per-strip kernel
    if (const int nv = to_yuv_strip_vectors(d.w, s.w, job.tx, job.ty)) {
        a.nv = nv;
        a.strips = (d.w + 63) / 64;
        a.rows = to_yuv_strip_rows((long)d.h * a.strips * job.n_pictures);
        a.chunks = (d.h + a.rows - 1) / a.rows;
        a.per_picture = a.strips * a.chunks;
        const long total = (long)a.per_picture * job.n_pictures;
        if (total > 0x3fffffff) return hipErrorInvalidValue;
        a.total = (int)total;
        dim3 grid((unsigned)(((a.total + 7) / 8) * 8));
        const size_t lds = (size_t)2 * nv * 16;                             // the two-row staging ring; the window is in registers
#define CHV_LY_GO(TT) hipLaunchKernelGGL(lanczos_yuv_strip<TT>, grid, dim3(64), lds, stream, a)
        switch (job.tx) {
        case 6: CHV_LY_GO(6); break;   case 8: CHV_LY_GO(8); break;   case 10: CHV_LY_GO(10); break; case 12: CHV_LY_GO(12); break;
        case 14: CHV_LY_GO(14); break; case 16: CHV_LY_GO(16); break; case 18: CHV_LY_GO(18); break; case 20: CHV_LY_GO(20); break;
        default: CHV_LY_GO(22); break;
        }
#undef CHV_LY_GO
        return hipGetLastError();
    }
    // the tile kernel (the shape: to_yuv_tile_shape)
    const size_t lds = to_yuv_tile_shape(d.h, s.h, job.ty, &a.tw, &a.max_rows);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    a.strips = (d.w + a.tw - 1) / a.tw;
    a.chunks = (d.h + YT_H - 1) / YT_H;
    a.per_picture = a.strips * a.chunks;
    const long total = (long)a.per_picture * job.n_pictures;
    if (total > 0x3fffffff) return hipErrorInvalidValue;
    a.total = (int)total;
    hipLaunchKernelGGL(lanczos_yuv_tile, dim3((unsigned)a.total), dim3(256), lds, stream, a);
    return hipGetLastError();
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosToYuvRegistrar { LanczosToYuvRegistrar() { register_lanczos_to_yuv_launcher(launch_lanczos_to_yuv); } } g_lanczos_to_yuv_registrar;

}  // namespace chv
