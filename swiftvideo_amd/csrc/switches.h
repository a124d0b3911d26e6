// switches.h — measurement / test switches of the path selection (host side only).
//
// The environment is read ONCE, at the first use in the process (getenv on a hot path is undefined behaviour next to a
// setenv in another thread, and the mixer and uploader threads run concurrently): CHV_FORCE_GENERAL, CHV_BGRA_PATH,
// CHV_WAVE_ROWS, CHV_TILE_ROWS, CHV_SAME_GEOM, CHV_DESC, CHV_STREAM, CHV_YUV_STREAM, CHV_WAVE_DMA, CHV_PASS_FUSE, CHV_GEOM_CACHE, CHV_STREAM_ROWS, CHV_STREAM_OPAQUE, CHV_STREAM_CARRY, CHV_STREAM_F32TAPS, CHV_STREAM_PLAN, CHV_REBIND.  Tests and A/B tools change them afterwards through chv_debug_set_switch (include/chipvideo.h),
// never through the environment.  Every value is an atomic int; 0 = "the library decides".
#pragma once
#include <atomic>

namespace chv {

struct Switches {
    std::atomic<int> force_general{0};   // 1: every tick through the general kernels
    std::atomic<int> bgra_path{0};       // 1: wave kernel also for one-YUV-layer BGRA ticks; 2: the tiled kernel wherever it applies
    std::atomic<int> wave_rows{0};       // 8 | 16: strip height of the wave kernels
    std::atomic<int> tile_rows{0};       // 16 | 32: tile height of the tiled YUV -> BGRA kernel
    std::atomic<int> same_geom{1};       // 0: do not share a layer's geometry with its predecessor (A/B of LF_SAME_GEOM)
    std::atomic<int> desc_host{0};       // CHV_DESC, a transient launch's descriptors: 0 kernel arguments where the kernel takes them (tick_bgra_stream_one), else a device
                                         // copy; 1 (host) read from the pinned host ring; 2 (device) the device copy always (A/Bs)
    std::atomic<int> stream{1};          // 0: never tick_bgra_stream (A/B; CHV_BGRA_PATH=stream: also for one-layer ticks)
    std::atomic<int> yuv_stream{1};      // CHV_YUV_STREAM: 0 never tick_yuv_stream (4:2:0 canvases keep tick_yuv_wave); 1 (default) where it measured faster
                                         // (tick_route.cpp::yuv_stream_eligible); force: every eligible launch (A/Bs and tests)
    std::atomic<int> wave_dma{1};        // CHV_WAVE_DMA: 0 the RGB-only strip kernel stages its rectangles through registers like the others (A/B, and the
                                         // fuzzers' way to the non-DMA staging of that instantiation); 1 (default) by LDS-DMA where the shape allows
    std::atomic<int> geom_cache{1};      // CHV_GEOM_CACHE: 0 the strip kernels compute every layer's per-strip geometry in place also in batches (A/B, and the
                                         // fuzzers' way to that path); 1 (default) batches keep it in tables built at their SECOND launch with a
                                         // configuration (geom_cache.h: a batch run once never pays); eager: at the first one (the test suite, whose
                                         // batches mostly run once, so that its fuzzers reach the table-reading kernels)
    std::atomic<int> pass_fuse{1};       // CHV_PASS_FUSE: 1 (default) picture kernels issued inside chv_pass_begin ... chv_pass_end are held and leave as the one
                                         // fused launch chv_composite would make of them (chipvideo.cpp: PendingPass); 0 every chv_run_kernel launches at once
    std::atomic<int> stream_rows{0};     // CHV_STREAM_ROWS: 1 .. 4096 canvas rows per chunk of tick_bgra_stream (tests: small launches take chunks of 4 .. 12 rows,
                                         // and the kernel's row table is refilled every 32); 0 (default) launch_bgra_stream decides
    std::atomic<int> stream_opaque{1};   // CHV_STREAM_OPAQUE: 0 launches whose bottom layers are all opaque keep tick_bgra_stream's general kernels (A/B and
                                         // parity tests); 1 (default) they take the opaque-bottom kernels (kernels_stream_opq.hip.cpp)
    std::atomic<int> stream_carry{1};    // CHV_STREAM_CARRY: 0 opaque-bottom launches keep the kernels that read every chroma tap on every row (A/B and parity
                                         // tests); 1 (default) NV12 batches whose chroma advances by at most one row per canvas row take the chroma-carry
                                         // kernels (kernels_stream_carry.hip.cpp; stream_select.h)
    std::atomic<int> stream_f32taps{1};  // CHV_STREAM_F32TAPS: 0 chroma-carry launches keep the kernels whose taps are v_fma_mix_f32 (A/B and parity tests); 1 (default)
                                         // they take the kernels whose taps are f32 multiply-adds on binary32 denormals (kernels_stream_dn.hip.cpp;
                                         // profiles/f32_denormal_taps_notes.md)
    std::atomic<int> stream_plan{1};     // CHV_STREAM_PLAN, how a batch launch of tick_bgra_stream is cut into waves (stream_plan.h): 0 one uniform chunk height always
                                         // (A/B and parity tests); 1 (default) batches whose tall phase alone fills the chip once run tall chunks first and short
                                         // ones at the end (profiles/stream_plan_notes.md); N >= 2 (tests) plan as if the chip held N waves and a tenth of a
                                         // round were enough, so that a batch of a few small ticks gets several phases
    std::atomic<int> rebind{0};          // CHV_REBIND, how chv_batch_rebind sends the new plane addresses: scatter (1) the scatter kernel (kernels_rebind.hip.cpp)
                                         // wherever the batch has a pooled block and the unit is linked; copy (2) the whole descriptor block again (A/B, and
                                         // the only way without them); 0 (default) the library decides (profiles/batch_rebind_notes.md)
};
Switches &switches();                    // (chipvideo.cpp; initialised from the environment on first use)

// Counters the launchers keep for tests and probes (chv_debug_get_counter; process-wide, relaxed).  Defined in chipvideo.cpp: the host units
// link without the kernel units (tests/stubhip), so the kernel units count here instead of exporting a reader.
struct DebugCounters {
    std::atomic<unsigned long long> stream_opaque_launches{0};       // launches of tick_bgra_stream that took the opaque-bottom kernels
    std::atomic<unsigned long long> stream_carry_launches{0};        // ... of which: the chroma-carry kernels (kernels_stream_carry.hip.cpp)
    std::atomic<unsigned long long> stream_f32tap_launches{0};       // ... of which: the f32-tap kernels (kernels_stream_dn.hip.cpp)
    std::atomic<unsigned long long> stream_phased_launches{0};       // launches of tick_bgra_stream cut into more than one phase (stream_plan.h)
    std::atomic<unsigned long long> lanczos_ladder_launches{0};      // device launches made by chv_scale_lanczos_to_yuv_ladder
    std::atomic<unsigned long long> lanczos_planar_ladder_launches{0};      // device launches made by chv_scale_lanczos_ladder
    std::atomic<unsigned long long> lanczos_420_ladder_launches{0};         // device launches made by the cross-format path of chv_scale_lanczos_420 / _420_ladder
    std::atomic<unsigned long long> lanczos_to_420_launches{0};             // device launches made by chv_scale_lanczos_to_420 / _to_420_ladder for the five formats they do not forward
    std::atomic<unsigned long long> lanczos_hbd_launches{0};                // device launches made by chv_scale_lanczos_hbd_to_420 / _hbd_to_420_ladder
    std::atomic<unsigned long long> lanczos_from_yuv_launches{0};           // device launches made by chv_scale_lanczos_from_yuv / _from_yuv_batch
    std::atomic<unsigned long long> lanczos_from_yuv_ladder_launches{0};    // device launches made by chv_scale_lanczos_from_yuv_ladder
    std::atomic<unsigned long long> lanczos_rgb_ladder_launches{0};         // device launches made by chv_scale_lanczos_rgb_ladder
};
DebugCounters &debug_counters();

}  // namespace chv
