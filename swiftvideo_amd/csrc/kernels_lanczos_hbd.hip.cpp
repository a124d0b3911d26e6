// kernels_lanczos_hbd.hip.cpp — Lanczos-3 from the two 10-bit 4:2:0 formats into the two 8-bit 4:2:0 packings (no
// reference counterpart): the renditions of one or several P010 or yuv420p10le pictures of one size as NV12 or y420p pictures of up to eight
// sizes, every rung in one launch per route.  chv_scale_lanczos_hbd_to_420 is the ladder of one rung and one picture.  The construction is
// lanczos_planar_ladder_body.hip.h's.  What differs per (source, target) cell is how a lane finds its source samples (hbd_strip's
// <tap stride, target components, two planes in a ring slot>):
//
//   source \ target plane   Y             CbCr of NV12                      Cb, Cr of y420p
//   P010                    <2, 1>        <4, 2>, offsets 0 / 2             <4, 1>, offset 0 or 2
//   y420p10                 <2, 1>        <2, 2, two planes>                <2, 1>
//
//   lanczos_hbd_ladder<MAXT, SRC>   the rungs that take the wave-per-strip route.  SRC: one row of the table (a kernel holds the bodies of one
//                                   source only, and with them its way from word to code), times two variants by the largest tap class among
//                                   the launch's strip rungs.
//   lanczos_hbd_ladder_tile         the rungs that take the tile route, every cell: hbd_tile with the cell's start pointers and tap stride.
#include "lanczos_hbd_body.hip.h"
#include "lanczos_hbd.h"
#include "lanczos_planar_ladder_body.hip.h"

namespace chv {

struct HbdArgs {
    const DPlane *batch;              // per picture: n_rungs * n_planes target planes, then the source's planes
    int32_t n_planes, per_image;      // TARGET planes of a picture (2: NV12, 3: y420p), planes of a picture's record
    int32_t src_at, rows;             // the source's first plane within a record; output rows per wave (strip route)
    int32_t source, pad;              // LanczosHbdSource
    int32_t first[kLanczosPlanarLadderMaxRungs];
    LadderRung420 rung[kLanczosPlanarLadderMaxRungs];
    // pl[].src: the LOGICAL image that feeds the plane (samples), comps its tap stride in bytes
    PlanarPlane pl[kLanczosPlanarLadderMaxRungs * kLanczosPlanarMaxPlanes];
};
static_assert(sizeof(HbdArgs) <= 4096 - 256, "kernel arguments: 4 KB in all, 256 bytes of them the runtime's");

struct HbdBlock {                     // (PlanarLadderBlock and src2)
    PlanarPlane g;                    // g.src: the logical image's size with the start and pitch of the plane that holds it
    DPlane src2;                      // the Cr plane of y420p10 when the target plane is CbCr; g.src otherwise
    int T, bx, by, plane;
    bool live;
};

// the source plane by the kind of source — P010: luma plane 0, chroma plane 1; y420p10: target plane p reads source plane p, a CbCr target
// planes 1 AND 2
template <bool XCD>
CHV_DEV HbdBlock hbd_decode(const HbdArgs &a, int blk) {
    return planar_ladder_block<XCD, HbdBlock>(a, blk, [](const HbdArgs &a, HbdBlock &o, uint64_t pic) {
        const int plane = o.plane, chroma = plane ? 1 : 0;
        const int pa = a.source == kHbdP010 || a.n_planes == 2 ? chroma : plane;
        const int pb = a.source == kHbdPlanar && a.n_planes == 2 && plane ? 2 : pa;
        const DPlane sa = cld<DPlane>(pic + (uint64_t)(a.src_at + pa) * sizeof(DPlane));
        o.src2 = cld<DPlane>(pic + (uint64_t)(a.src_at + pb) * sizeof(DPlane));
        o.g.src.ptr = sa.ptr; o.g.src.pitch = sa.pitch;            // (w, h: the logical image's, from the launch's record)
    });
}

template <int T, int SRC>
CHV_DEV void hbd_cell(const HbdArgs &a, const HbdBlock &blk, uint8_t *lsm) {
    const bool luma = blk.plane == 0, nv12 = a.n_planes == 2;     // (uniform)
    if constexpr (SRC == kHbdP010) {
        if (luma) hbd_strip<T, 2, 1, false, kSampleHigh10>(blk.g, blk.src2, 0, 0, blk.bx, blk.by, a.rows, lsm);
        else if (nv12) hbd_strip<T, 4, 2, false, kSampleHigh10>(blk.g, blk.src2, 0, 2, blk.bx, blk.by, a.rows, lsm);
        else hbd_strip<T, 4, 1, false, kSampleHigh10>(blk.g, blk.src2, blk.plane == 1 ? 0 : 2, 0, blk.bx, blk.by, a.rows, lsm);
    } else {
        if (luma || !nv12) hbd_strip<T, 2, 1, false, kSampleLow10>(blk.g, blk.src2, 0, 0, blk.bx, blk.by, a.rows, lsm);
        // even lanes read the first half of the ring slot (Cb's row), odd lanes the second (Cr's), nv vectors on
        else hbd_strip<T, 2, 2, true, kSampleLow10>(blk.g, blk.src2, 0, blk.g.nv * 16, blk.bx, blk.by, a.rows, lsm);
    }
}

template <int MAXT, int SRC>
__global__ __launch_bounds__(64, (MAXT <= 12 ? 5 : 4)) void lanczos_hbd_ladder(const HbdArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t hbd_lsm[];
    const HbdBlock blk = hbd_decode<true>(a, blockIdx.x);
    if (!blk.live) return;
#define CHV_HBD_CASE(TT) case TT: if constexpr (TT <= MAXT) hbd_cell<TT, SRC>(a, blk, hbd_lsm); break
    switch (blk.T) {                  // (uniform)
    CHV_HBD_CASE(6); CHV_HBD_CASE(8); CHV_HBD_CASE(12); CHV_HBD_CASE(16); CHV_HBD_CASE(22);
    default: break;
    }
#undef CHV_HBD_CASE
}

__global__ __launch_bounds__(256) void lanczos_hbd_ladder_tile(const HbdArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t hbd_lsm[];
    const HbdBlock blk = hbd_decode<false>(a, blockIdx.x);
    if (!blk.live) return;
    const bool p010 = a.source == kHbdP010;
    // the start of component 0's (or the only component's) samples, of component 1's, and the bytes between two samples
    const int stride = p010 && blk.plane ? 4 : 2;
    const int oa = p010 && blk.plane == 2 ? 2 : 0, ob = p010 ? 2 : 0;
    hbd_tile(blk.g, blk.g.src.ptr + oa, blk.g.src.pitch, blk.src2.ptr + ob, blk.src2.pitch, stride, p010 ? 6 : 0, blk.bx, blk.by, hbd_lsm);
}

template <int SRC>
static void hbd_launch_strip(bool small, unsigned grid, size_t lds, hipStream_t stream, const HbdArgs &a) {
    if (small) hipLaunchKernelGGL((lanczos_hbd_ladder<12, SRC>), dim3(grid), dim3(64), lds, stream, a);
    else hipLaunchKernelGGL((lanczos_hbd_ladder<22, SRC>), dim3(grid), dim3(64), lds, stream, a);
}

static hipError_t launch_lanczos_hbd(const LanczosHbdJob &job, hipStream_t stream, int *launches) {
    *launches = 0;
    const int np = job.dst_planes;
    const bool to_nv12 = np == 2, p010 = job.source == kHbdP010;
    if ((np != 2 && np != 3) || (job.source != kHbdP010 && job.source != kHbdPlanar) || job.src_planes != (p010 ? 2 : 3) || job.n_pictures < 1 ||
        job.n_rungs < 1 || job.n_rungs > kLanczosPlanarLadderMaxRungs || !job.batch)
        return hipErrorInvalidValue;
    HbdArgs proto{};
    proto.batch = job.batch; proto.n_planes = np; proto.per_image = job.n_rungs * np + job.src_planes; proto.src_at = job.n_rungs * np;
    proto.source = job.source;
    const auto plane = [&](int r, int p) {
        const Lanczos420Rung &j = job.rung[r];
        return planar_ladder_plane(j.tab[p], DPlane{ nullptr, j.w[p], j.h[p], 0, to_nv12 && p == 1 ? 2 : 1 },
                                   DPlane{ nullptr, p ? job.chroma_w : job.luma_w, p ? job.chroma_h : job.luma_h, 0, hbd_tap_stride(job.source, p) });
    };
    PlanarLadderPlan<HbdArgs> L;
    if (!planar_ladder_plan(&L, proto, job.n_rungs, np, job.n_pictures, plane, p010 ? hbd_strip_route_p010 : hbd_strip_route_planar)) return hipErrorInvalidValue;
    return ladder_launch(launches, L.n_strip, [&] {
        if (p010) hbd_launch_strip<kHbdP010>(L.max_t <= 12, L.strip_grid, L.strip_lds, stream, L.strip);
        else hbd_launch_strip<kHbdPlanar>(L.max_t <= 12, L.strip_grid, L.strip_lds, stream, L.strip);
    }, L.n_tile, [&] { hipLaunchKernelGGL(lanczos_hbd_ladder_tile, dim3(L.tile_grid), dim3(256), L.tile_lds, stream, L.tile); });
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct LanczosHbdRegistrar { LanczosHbdRegistrar() { register_lanczos_hbd_launcher(launch_lanczos_hbd); } } g_lanczos_hbd_registrar;

}  // namespace chv
