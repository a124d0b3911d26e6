// chipvideo.cpp — host runtime behind include/chipvideo.h.
//
// Owns devices, contexts (one HIP stream each), device buffers, pitched
// transfers with a pinned staging ring, descriptor building/validation and
// kernel dispatch.  There is no CPU pixel path in this library: every entry
// that would touch pixels either launches a gfx950 kernel or returns an error.
#include "../../include/chipvideo.h"

#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdarg>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "device_types.h"
#include "switches.h"
#include "tick_route.h"
#include "geom_cache.h"
#include "rebind.h"
#include "lanczos_planar.h"
#include "lanczos_to_yuv.h"
#include "lanczos_ladder.h"
#include "lanczos_planar_ladder.h"
#include "lanczos_420.h"
#include "lanczos_to_420.h"
#include "lanczos_hbd.h"
#include "lanczos_from_yuv.h"
#include "lanczos_from_yuv_ladder.h"
#include "lanczos_rgb_ladder.h"

namespace chv {
const char *bgra_wave_build_flags();      // kernels_wave.hip.cpp
const char *yuv_wave_build_flags();       // kernels_wave_yuv.hip.cpp
const char *bgra_stream_build_flags();   // kernels_stream.hip.cpp
const char *yuv_stream_build_flags();    // kernels_stream_yuv.hip.cpp
const char *lanczos_build_flags();       // kernels_lanczos.hip.cpp
hipError_t launch_tick_general(int target_format, const DTick *ticks_host, const DLayer *layers_host, const DTick *ticks, const DLayer *layers,
                               int n_ticks, int maxW, int maxH, hipStream_t stream);
hipError_t launch_selftest(float *out_f, const float *in_f, uint8_t *out_c, const float *num,
                           const float *den, float *out_q, int n, hipStream_t stream);
hipError_t launch_selftest_pack(const int *b, const int *g, const int *r, uint32_t *out, int n, hipStream_t stream);
hipError_t launch_selftest_pack_codes(const float *in, uint32_t *out, int n, hipStream_t stream);
hipError_t launch_selftest_matrices(int dir, int csc, uint32_t *out, uint32_t *mism, hipStream_t stream);
// kernels_fast.hip.cpp (the routes it launches: tick_route.h)
// tables: the launch's geometry tables for the strip kernels (geom_cache.h; nullptr: none — they compute their geometry in place)
hipError_t launch_tick_fast(int path, const DTick *ticks_host, const DLayer *layers_host,
                            const DTick *ticks, const DLayer *layers, int n_ticks,
                            int maxW, int maxH, hipStream_t stream, GeomCache *tables);
// kernels_idle.hip.cpp
hipError_t launch_snd_s16i(int16_t *out, const int16_t *const *in, int count, int n, const float *gain, const float *fade, hipStream_t stream);
hipError_t launch_me_fullsearch(const DPlane &out, const DPlane &ref, const DPlane &cur, const int32_t *block, const int32_t *window, const int32_t *image,
                                const float *cost256, hipStream_t stream);
// kernels_lanczos.hip.cpp
hipError_t launch_lanczos(const DPlane &dst, const DPlane &src, const int32_t *fx, const float *wx,
                          int tx, const int32_t *fy, const float *wy, int ty, hipStream_t stream,
                          const DPlane *batch, int n_batch, int stride_x, int first_x, int stride_y);
}  // namespace chv

using namespace chv;

static void g_detail_set(const char *msg);

// ---------------------------------------------------------------------------
// switches (switches.h) and build flags
// ---------------------------------------------------------------------------
static int parse_switch(const char *name, const char *value, int *out) {
    const std::string n = name ? name : "", v = value ? value : "";
    if (n == "CHV_FORCE_GENERAL") { *out = v == "1" ? 1 : 0; return 0; }
    if (n == "CHV_BGRA_PATH") { *out = v == "wave" ? 1 : v == "tiled" ? 2 : v == "stream" ? 3 : 0; return 1; }
    if (n == "CHV_WAVE_ROWS") { *out = v == "8" ? 8 : v == "16" ? 16 : 0; return 2; }
    if (n == "CHV_TILE_ROWS") { *out = v == "16" ? 16 : v == "32" ? 32 : 0; return 3; }
    if (n == "CHV_SAME_GEOM") { *out = v == "0" ? 0 : 1; return 4; }
    if (n == "CHV_DESC") { *out = v == "host" ? 1 : v == "device" ? 2 : 0; return 5; }
    if (n == "CHV_STREAM") { *out = v == "0" ? 0 : 1; return 6; }
    if (n == "CHV_YUV_STREAM") { *out = v == "0" ? 0 : (v == "force" || v == "2") ? 2 : 1; return 7; }
    if (n == "CHV_WAVE_DMA") { *out = v == "0" ? 0 : 1; return 8; }
    if (n == "CHV_PASS_FUSE") { *out = v == "0" ? 0 : 1; return 9; }
    if (n == "CHV_GEOM_CACHE") { *out = v == "0" ? 0 : v == "eager" ? 2 : 1; return 10; }
    if (n == "CHV_STREAM_ROWS") { const int r = atoi(v.c_str()); *out = (r >= 1 && r <= 4096) ? r : 0; return 11; }
    if (n == "CHV_STREAM_OPAQUE") { *out = v == "0" ? 0 : 1; return 12; }
    if (n == "CHV_STREAM_CARRY") { *out = v == "0" ? 0 : 1; return 14; }
    if (n == "CHV_REBIND") { *out = v == "scatter" ? 1 : v == "copy" ? 2 : 0; return 13; }
    if (n == "CHV_STREAM_F32TAPS") { *out = v == "0" ? 0 : 1; return 15; }
    if (n == "CHV_STREAM_PLAN") { const int r = atoi(v.c_str()); *out = v == "0" ? 0 : (r >= 2 && r <= (1 << 24)) ? r : 1; return 16; }
    return -1;
}
static void store_switch(Switches &s, int which, int val) {
    std::atomic<int> *slots[17] = { &s.force_general, &s.bgra_path, &s.wave_rows, &s.tile_rows, &s.same_geom, &s.desc_host, &s.stream, &s.yuv_stream, &s.wave_dma,
                                    &s.pass_fuse, &s.geom_cache, &s.stream_rows, &s.stream_opaque, &s.rebind, &s.stream_carry, &s.stream_f32taps, &s.stream_plan };
    slots[which]->store(val, std::memory_order_relaxed);
}
Switches &chv::switches() {
    static Switches s;
    static std::once_flag once;
    std::call_once(once, [] {
        static const char *const names[17] = { "CHV_FORCE_GENERAL", "CHV_BGRA_PATH", "CHV_WAVE_ROWS", "CHV_TILE_ROWS", "CHV_SAME_GEOM", "CHV_DESC", "CHV_STREAM", "CHV_YUV_STREAM",
                                               "CHV_WAVE_DMA", "CHV_PASS_FUSE", "CHV_GEOM_CACHE", "CHV_STREAM_ROWS", "CHV_STREAM_OPAQUE", "CHV_REBIND", "CHV_STREAM_CARRY", "CHV_STREAM_F32TAPS", "CHV_STREAM_PLAN" };
        for (const char *n : names) {
            const char *v = getenv(n);
            int val = 0, which = v ? parse_switch(n, v, &val) : -1;
            if (which >= 0) store_switch(s, which, val);
        }
    });
    return s;
}
// the scatter kernel's launcher (rebind.h): null until kernels_rebind.hip.cpp registers it, and for good in a build without that unit
static std::atomic<RebindLauncher> g_rebind_launcher{nullptr};
void chv::register_rebind_launcher(RebindLauncher fn) { g_rebind_launcher.store(fn, std::memory_order_release); }
// the planar Lanczos launcher (lanczos_planar.h): null until kernels_lanczos_planar.hip.cpp registers it, and for good in a build without that unit
static std::atomic<LanczosPlanarLauncher> g_lanczos_planar_launcher{nullptr};
void chv::register_lanczos_planar_launcher(LanczosPlanarLauncher fn) { g_lanczos_planar_launcher.store(fn, std::memory_order_release); }
// the same for chv_scale_lanczos_to_yuv (lanczos_to_yuv.h, kernels_lanczos_to_yuv.hip.cpp)
static std::atomic<LanczosToYuvLauncher> g_lanczos_to_yuv_launcher{nullptr};
void chv::register_lanczos_to_yuv_launcher(LanczosToYuvLauncher fn) { g_lanczos_to_yuv_launcher.store(fn, std::memory_order_release); }
// and for chv_scale_lanczos_to_yuv_ladder (lanczos_ladder.h, kernels_lanczos_ladder.hip.cpp)
static std::atomic<LanczosLadderLauncher> g_lanczos_ladder_launcher{nullptr};
void chv::register_lanczos_ladder_launcher(LanczosLadderLauncher fn) { g_lanczos_ladder_launcher.store(fn, std::memory_order_release); }
// and for chv_scale_lanczos_ladder (lanczos_planar_ladder.h, kernels_lanczos_planar_ladder.hip.cpp)
static std::atomic<LanczosPlanarLadderLauncher> g_lanczos_planar_ladder_launcher{nullptr};
void chv::register_lanczos_planar_ladder_launcher(LanczosPlanarLadderLauncher fn) { g_lanczos_planar_ladder_launcher.store(fn, std::memory_order_release); }
// and for the cross pairs of chv_scale_lanczos_420 / chv_scale_lanczos_420_ladder (lanczos_420.h, kernels_lanczos_420.hip.cpp)
static std::atomic<Lanczos420Launcher> g_lanczos_420_launcher{nullptr};
void chv::register_lanczos_420_launcher(Lanczos420Launcher fn) { g_lanczos_420_launcher.store(fn, std::memory_order_release); }
// and for the five other decoder formats of chv_scale_lanczos_to_420 / chv_scale_lanczos_to_420_ladder (lanczos_to_420.h, kernels_lanczos_to_420.hip.cpp)
static std::atomic<LanczosTo420Launcher> g_lanczos_to_420_launcher{nullptr};
void chv::register_lanczos_to_420_launcher(LanczosTo420Launcher fn) { g_lanczos_to_420_launcher.store(fn, std::memory_order_release); }
// and for the 10-bit sources of chv_scale_lanczos_hbd_to_420 / chv_scale_lanczos_hbd_to_420_ladder (lanczos_hbd.h, kernels_lanczos_hbd.hip.cpp)
static std::atomic<LanczosHbdLauncher> g_lanczos_hbd_launcher{nullptr};
void chv::register_lanczos_hbd_launcher(LanczosHbdLauncher fn) { g_lanczos_hbd_launcher.store(fn, std::memory_order_release); }
// and for chv_scale_lanczos_from_yuv / chv_scale_lanczos_from_yuv_batch (lanczos_from_yuv.h, kernels_lanczos_from_yuv.hip.cpp)
static std::atomic<LanczosFromYuvLauncher> g_lanczos_from_yuv_launcher{nullptr};
void chv::register_lanczos_from_yuv_launcher(LanczosFromYuvLauncher fn) { g_lanczos_from_yuv_launcher.store(fn, std::memory_order_release); }
// and for chv_scale_lanczos_from_yuv_ladder (lanczos_from_yuv_ladder.h, kernels_lanczos_from_yuv_ladder.hip.cpp)
static std::atomic<LanczosFromYuvLadderLauncher> g_lanczos_from_yuv_ladder_launcher{nullptr};
void chv::register_lanczos_from_yuv_ladder_launcher(LanczosFromYuvLadderLauncher fn) { g_lanczos_from_yuv_ladder_launcher.store(fn, std::memory_order_release); }
// and for chv_scale_lanczos_rgb_ladder (lanczos_rgb_ladder.h, kernels_lanczos_rgb_ladder.hip.cpp)
static std::atomic<LanczosRgbLadderLauncher> g_lanczos_rgb_ladder_launcher{nullptr};
void chv::register_lanczos_rgb_ladder_launcher(LanczosRgbLadderLauncher fn) { g_lanczos_rgb_ladder_launcher.store(fn, std::memory_order_release); }
DebugCounters &chv::debug_counters() {
    static DebugCounters c;
    return c;
}
extern "C" int chv_debug_set_switch(const char *name, const char *value) {
    int val = 0;
    Switches &s = switches();                     // (environment first, so that a later first use cannot overwrite this)
    const int which = parse_switch(name, value, &val);
    if (which < 0) { g_detail_set("unknown switch"); return CHV_ERR_INVALID_VALUE; }
    if (!value || !*value) val = (which == 4 || which == 6 || which == 7 || which == 8 || which == 9 || which == 10 || which == 12 || which == 14 || which == 15 || which == 16) ? 1 : 0;      // empty / NULL: back to "the library decides"
    store_switch(s, which, val);
    return CHV_OK;
}
extern "C" int chv_debug_get_counter(const char *name, unsigned long long *value) {
    static const char *const names[] = { "geom_store_patched", "geom_store_batch_hits", "geom_store_builds", "geom_store_bytes", "geom_store_tables" };
    if (!name || !value) { g_detail_set("null argument"); return CHV_ERR_INVALID_VALUE; }
    for (int i = 0; i < 5; i++)
        if (!strcmp(name, names[i])) { *value = (unsigned long long)geom_store_counter(i); return CHV_OK; }
    if (!strcmp(name, "stream_opaque_launches")) { *value = debug_counters().stream_opaque_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "stream_carry_launches")) { *value = debug_counters().stream_carry_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "stream_f32tap_launches")) { *value = debug_counters().stream_f32tap_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "stream_phased_launches")) { *value = debug_counters().stream_phased_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "lanczos_planar_ladder_launches")) { *value = debug_counters().lanczos_planar_ladder_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "lanczos_420_ladder_launches")) { *value = debug_counters().lanczos_420_ladder_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "lanczos_to_420_launches")) { *value = debug_counters().lanczos_to_420_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "lanczos_hbd_launches")) { *value = debug_counters().lanczos_hbd_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "lanczos_from_yuv_launches")) { *value = debug_counters().lanczos_from_yuv_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "lanczos_from_yuv_ladder_launches")) { *value = debug_counters().lanczos_from_yuv_ladder_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "lanczos_rgb_ladder_launches")) { *value = debug_counters().lanczos_rgb_ladder_launches.load(std::memory_order_relaxed); return CHV_OK; }
    if (!strcmp(name, "lanczos_ladder_launches")) { *value = debug_counters().lanczos_ladder_launches.load(std::memory_order_relaxed); return CHV_OK; }
    g_detail_set("unknown counter");
    return CHV_ERR_INVALID_VALUE;
}
extern "C" const char *chv_build_flags(void) {
    // what the library was built with: the architecture the Makefile compiled for, the compiler (the hand-scheduled kernels — LDS-DMA through
    // M0, counted vmcnt waits, prefetch registers in flight — were validated against THIS hipcc; tests/test_device_code_contract.py refuses
    // another major version until tools/check_inflight.py and the GPU suite have been re-run with it), every timing-only ablation macro
    static const std::string flags = std::string("arch=" CHV_ARCH ";hipcc=" CHV_HIPCC_VERSION ";clang=") + std::to_string(__clang_major__) + "." + std::to_string(__clang_minor__) +
                                     ";fp_contract=off;" + bgra_wave_build_flags() + ";" + yuv_wave_build_flags() + ";" + bgra_stream_build_flags() + ";" +
                                     yuv_stream_build_flags() + ";" + lanczos_build_flags() +
                                     (g_rebind_launcher.load(std::memory_order_acquire) ? ";batch_rebind:scatter=1" : ";batch_rebind:scatter=0");
    return flags.c_str();
}

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_detail;
static void g_detail_set(const char *msg) { g_detail = msg; }

static int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_detail = buf;
    return code;
}

// HIP error -> ComputeError-shaped status (the role of check(), compute.cuda.swift:102-112)
static int hip_fail(hipError_t e, const char *what) {
    int code = CHV_ERR_UNKNOWN;
    switch (e) {
    case hipErrorOutOfMemory: code = CHV_ERR_OUT_OF_MEMORY; break;
    case hipErrorInvalidValue: code = CHV_ERR_INVALID_VALUE; break;
    case hipErrorInvalidDevice: code = CHV_ERR_INVALID_DEVICE; break;
    case hipErrorNoDevice: code = CHV_ERR_DEVICE_NOT_AVAILABLE; break;
    case hipErrorInvalidContext: code = CHV_ERR_INVALID_CONTEXT; break;
    case hipErrorNotSupported: code = CHV_ERR_NOT_IMPLEMENTED; break;
    default: break;
    }
    return fail(code, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
}
#define HIP_TRY(expr)                                         \
    do {                                                      \
        hipError_t _e = (expr);                               \
        if (_e != hipSuccess) return hip_fail(_e, #expr);     \
    } while (0)

extern "C" const char *chv_error_string(int s) {
    switch (s) {
    case CHV_OK: return "success";
    case CHV_ERR_INVALID_VALUE: return "invalidValue";
    case CHV_ERR_OUT_OF_MEMORY: return "outOfMemory";
    case CHV_ERR_INVALID_CONTEXT: return "invalidContext";
    case CHV_ERR_BAD_TARGET: return "badTarget";
    case CHV_ERR_BAD_INPUT: return "badInputData";
    case CHV_ERR_NOT_IMPLEMENTED: return "notImplemented";
    case CHV_ERR_KERNEL_NOT_FOUND: return "computeKernelNotFound";
    case CHV_ERR_DEVICE_NOT_AVAILABLE: return "deviceNotAvailable";
    case CHV_ERR_INVALID_DEVICE: return "invalidDevice";
    case CHV_ERR_INVALID_OPERATION: return "invalidOperation";
    case CHV_ERR_BAD_CONTEXT_STATE: return "badContextState";
    case CHV_ERR_INVALID_PLATFORM: return "invalidPlatform";
    default: return "unknownError";
    }
}
extern "C" const char *chv_last_error_detail(void) { return g_detail.c_str(); }
extern "C" int chv_version(void) { return CHV_VERSION; }

// ---------------------------------------------------------------------------
// kernel name table (defaultComputeKernelFromString, compute.swift:90-110)
// ---------------------------------------------------------------------------
struct KernelName { const char *name; int id; };
static const KernelName kNames[] = {
    { "img_nv12_nv12", CHV_K_IMG_NV12_NV12 },   { "img_bgra_nv12", CHV_K_IMG_BGRA_NV12 },
    { "img_rgba_nv12", CHV_K_IMG_RGBA_NV12 },   { "img_bgra_bgra", CHV_K_IMG_BGRA_BGRA },
    { "img_y420p_y420p", CHV_K_IMG_Y420P_Y420P }, { "img_y420p_nv12", CHV_K_IMG_Y420P_NV12 },
    { "img_clear_nv12", CHV_K_IMG_CLEAR_NV12 }, { "img_clear_yuvs", CHV_K_IMG_CLEAR_YUVS },
    { "img_clear_bgra", CHV_K_IMG_CLEAR_BGRA }, { "img_clear_rgba", CHV_K_IMG_CLEAR_BGRA },
    { "img_rgba_y420p", CHV_K_IMG_RGBA_Y420P }, { "img_bgra_y420p", CHV_K_IMG_BGRA_Y420P },
    { "img_clear_y420p", CHV_K_IMG_CLEAR_Y420P },
    // names findKernel can synthesise for BGRA canvases (mix.video.swift:142-146)
    { "img_nv12_bgra", CHV_K_IMG_NV12_BGRA },   { "img_y420p_bgra", CHV_K_IMG_Y420P_BGRA },
    { "img_bgra_bgra_tx", CHV_K_IMG_BGRA_BGRA_TX }, { "img_rgba_bgra_tx", CHV_K_IMG_RGBA_BGRA_TX },
    // an RGBA layer on a BGRA canvas: no reference backend has a kernel of that name; it resolves to the transform-aware
    // one (as "img_clear_rgba" resolves to img_clear_bgra, compute.swift:101)
    { "img_rgba_bgra", CHV_K_IMG_RGBA_BGRA_TX },
    { "img_bgra_nv12_int", CHV_K_IMG_BGRA_NV12_INT }, { "img_rgba_nv12_int", CHV_K_IMG_RGBA_NV12_INT },
    { "img_bgra_y420p_int", CHV_K_IMG_BGRA_Y420P_INT }, { "img_rgba_y420p_int", CHV_K_IMG_RGBA_Y420P_INT },
    // the two cases of the enum the reference's table leaves out (compute.swift:91-105; nothing dispatches them there): resolvable here, so that
    // every case that has a kernel can be asked for by its name
    { "snd_s16i_s16i", CHV_K_SND_S16I_S16I }, { "me_fullsearch", CHV_K_ME_FULLSEARCH },
};

extern "C" int chv_kernel_from_string(const char *name, int *kernel) {
    if (!name || !kernel) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    for (const auto &k : kNames)
        if (!strcmp(k.name, name)) { *kernel = k.id; return CHV_OK; }
    return fail(CHV_ERR_INVALID_VALUE, "no default kernel named '%s'", name);
}

extern "C" const char *chv_kernel_name(int kernel) {
    switch (kernel) {
    case CHV_K_IMG_NV12_NV12: return "img_nv12_nv12";
    case CHV_K_IMG_BGRA_NV12: return "img_bgra_nv12";
    case CHV_K_IMG_RGBA_NV12: return "img_rgba_nv12";
    case CHV_K_IMG_BGRA_BGRA: return "img_bgra_bgra";
    case CHV_K_IMG_Y420P_Y420P: return "img_y420p_y420p";
    case CHV_K_IMG_Y420P_NV12: return "img_y420p_nv12";
    case CHV_K_IMG_CLEAR_NV12: return "img_clear_nv12";
    case CHV_K_IMG_CLEAR_YUVS: return "img_clear_yuvs";
    case CHV_K_IMG_CLEAR_BGRA: return "img_clear_bgra";
    case CHV_K_IMG_CLEAR_Y420P: return "img_clear_y420p";
    case CHV_K_IMG_CLEAR_RGBA: return "img_clear_rgba";
    case CHV_K_IMG_RGBA_Y420P: return "img_rgba_y420p";
    case CHV_K_IMG_BGRA_Y420P: return "img_bgra_y420p";
    case CHV_K_SND_S16I_S16I: return "snd_s16i_s16i";
    case CHV_K_ME_FULLSEARCH: return "me_fullsearch";
    case CHV_K_IMG_NV12_BGRA: return "img_nv12_bgra";
    case CHV_K_IMG_Y420P_BGRA: return "img_y420p_bgra";
    case CHV_K_IMG_BGRA_BGRA_TX: return "img_bgra_bgra_tx";
    case CHV_K_IMG_RGBA_BGRA_TX: return "img_rgba_bgra_tx";
    case CHV_K_IMG_BGRA_NV12_INT: return "img_bgra_nv12_int";
    case CHV_K_IMG_RGBA_NV12_INT: return "img_rgba_nv12_int";
    case CHV_K_IMG_BGRA_Y420P_INT: return "img_bgra_y420p_int";
    case CHV_K_IMG_RGBA_Y420P_INT: return "img_rgba_y420p_int";
    default: return NULL;
    }
}

// ---------------------------------------------------------------------------
// objects
// ---------------------------------------------------------------------------
// Device-side Lanczos tables of one (in, out) size pair.  Shared ownership: the cache holds one reference, every call that
// looked the pair up holds another until its launch is enqueued — an eviction by another context of the device can therefore
// never free tables between a lookup and the launch that reads them.  The memory goes back with hipFree, which waits for the
// work already queued on the device (i.e. for the launches that read the tables).
struct LanczosTable {
    int device = 0;
    int taps = 0;
    int32_t *first = nullptr;  // device
    float *weights = nullptr;  // device
    int stride = 0;            // first[o + 1] - first[o] when that is the same for every o (2 for the 2:1 class), else 0
    int first0 = 0;            // first[0]
    LanczosTable() = default;
    LanczosTable(const LanczosTable &) = delete;
    LanczosTable &operator=(const LanczosTable &) = delete;
    ~LanczosTable() {
        if (first || weights) { (void)hipSetDevice(device); (void)hipFree(first); (void)hipFree(weights); }
    }
};
typedef std::shared_ptr<LanczosTable> LanczosRef;
struct LanczosEntry {
    LanczosRef tab;
    uint64_t last_use = 0;     // LRU stamp
};
static constexpr size_t kLanczosCacheEntries = 64;   // (in, out) size pairs kept per device; least recently used goes first
static constexpr size_t kLanczosRetireBatch = 32;    // evicted tables are freed this many at a time (hipFree synchronises the device)

// State shared by a context and everything created with chv_context_share
// (the role of InternalContext, compute.cl.swift:60-74).
struct DeviceShared {
    int device = 0;
    std::mutex mu;
    std::map<std::pair<int, int>, LanczosEntry> lanczos;  // (in, out) -> tables
    std::vector<LanczosRef> lanczos_retired;               // evicted, not yet freed (see lanczos_table)
    uint64_t lanczos_clock = 0;
    ~DeviceShared() { (void)hipSetDevice(device); }         // (the tables free themselves)
};

// A run-time compiled kernel (`ComputeKernel.custom`): the module lives as long as any context's library names it.
struct CustomKernel {
    int device = 0;
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    ~CustomKernel() {
        if (module) { (void)hipSetDevice(device); (void)hipModuleUnload(module); }
    }
};

struct StagingSlot {
    void *host = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
};

// The descriptor ring is walked slot by slot, and its slots are guarded in GROUPS of kDescGroup: one event after the launch that used a
// group's last slot stands for every launch of the group (a stream runs in order), and it is waited for when the walk enters the group
// again, kDescSlots launches later.  An event per launch — what this was until round 3 — put a marker between every two kernels of a
// tick issued layer by layer: an unchanged mix.video.swift tick (clear + 4 launches + wait) took 77-84 us with them and 55 without.
struct DescGroup {
    hipEvent_t done = nullptr;
    bool pending = false;     // `done` has been recorded and not yet waited for
    bool unguarded = false;   // the event behind the group's last slot could not be recorded: the walk drains the stream before it enters the group again
};

static constexpr int kStagingSlots = 4;
static constexpr int kDescSlots = 64, kDescGroup = 8;
static constexpr size_t kDescSlotBytes = sizeof(DTick) + CHV_MAX_LAYERS * sizeof(DLayer);

struct chv_context {
    uint32_t magic = 0x43485643;  // 'CHVC'
    int device = 0;
    hipStream_t stream = nullptr;
    std::shared_ptr<DeviceShared> shared;
    int pass_depth = 0;                // open chv_pass_begin brackets (an upload helper that brackets its copies inside the mixer's pass nests)
    StagingSlot staging[kStagingSlots];
    int next_staging = 0;
    // descriptor ring in pinned, device-mapped host memory
    uint8_t *desc_host = nullptr;
    uint8_t *desc_dev = nullptr;       // the same ring in device memory: a transient launch's descriptors are copied there on the stream
    DescGroup desc_group[kDescSlots / kDescGroup];
    int next_desc = 0;
    // `library` of the reference's ComputeContext (compute.cl.swift:66-73): name -> built kernel
    std::map<std::string, std::shared_ptr<CustomKernel>> library;
    // The picture kernels of the pass in progress that have been accepted but not launched yet (PendingPass below): inside
    // chv_pass_begin ... chv_pass_end nothing has to be visible before the pass ends, so `clear + N layer kernels on one target` — what an
    // unchanged VideoMixer issues per tick, mix.video.swift:116-124 — leaves as the ONE launch chv_composite would have made of it.
    struct PendingPass {
        bool active = false;
        chv_image target;
        int clear_first = 0;
        int clear_tf = -1;                     // the target format a clear kernel fixed (kernel_shape), -1: the layers decide
        std::vector<chv_layer> layers;         // POD copies: the caller's structs need not outlive chv_run_kernel
        std::vector<chv_buffer *> pins;        // every buffer the pending kernels name, held against chv_buffer_free until they are launched
    } pending;
};

struct chv_buffer {
    uint32_t magic = 0x43485642;  // 'CHVB'
    void *ptr = nullptr;
    size_t size = 0;
    int device = 0;
    bool owned = true;
    // cross-context ordering: an asynchronous upload records `ready` on the uploading
    // context's stream; a kernel launched from another context's stream waits on it first
    // (the reference gets this ordering from blocking copies, compute.cl.swift:440-450)
    // (guarded by `mu`: the uploading thread and the launching thread are different threads in the reference's
    // pipeline — a Bus runner and the mixer's queue)
    std::mutex mu;
    hipEvent_t ready = nullptr;
    std::atomic<hipStream_t> ready_stream{nullptr};      // (atomic: launches look without the lock first — most buffers have nothing pending)
    uint64_t ready_seq = 0;
    // Deferred passes (chv_context::PendingPass): kernels that were accepted but not launched yet hold their buffers.  chv_buffer_free on a held
    // buffer marks it `doomed` and returns; the release that drops the last hold frees it (OpenCL keeps a cl_mem alive the same way from
    // clSetKernelArg / enqueue to completion — a ComputeBuffer's deinit may run the moment runComputeKernel returns, compute.cl.swift:55-57).
    // Both fields are guarded by g_pin_mu.
    int pins = 0;
    bool doomed = false;
};
static std::mutex g_pin_mu;
// (passes and kernels, below) launch what the pass in progress has accepted so far; every entry point that touches the context's stream starts with it
static int flush_pending(chv_context *c);
#define FLUSH_PENDING(c) do { if ((c)->pending.active) { int frc_ = flush_pending(c); if (frc_) return frc_; } } while (0)

// after an asynchronous copy into `b` was enqueued on `stream`: record the buffer's event
static int mark_uploaded(chv_buffer *b, hipStream_t stream);
// before `stream` reads or overwrites `b`: wait (on the stream, not on the host) for a pending upload from another stream
static int wait_for_buffer(chv_buffer *b, hipStream_t stream);

struct chv_event {
    hipEvent_t ev = nullptr;
    int device = 0;
};

struct BatchDep {
    chv_buffer *buf;
    hipStream_t stream;   // the stream that last waited for this buffer on behalf of the batch
    uint64_t seq;         // ... and the upload it saw
};

// ---- descriptor blocks of batches -----------------------------------------------------------------------------------------------------------
// A host that groups its mixers builds a batch for every group tick, runs it once and frees it (tools/batch_create_probe.cpp): two hipMalloc, two
// synchronous copies and two hipFree (which wait for the device) per tick were 45 of the 105 us a group of eight ticks took.  A batch's
// descriptors — ticks | layers | the second launch's ticks — now live in ONE block of a per-device pool: device memory with a pinned host twin
// and an event.  Creation fills the twin and sends it with one asynchronous copy on the creating context's stream; every run records the
// block's event behind its launches (a run on another stream first makes that stream wait for it); a block taken from the pool again waits
// for its event on the host before the twin is overwritten (a host that waited for its tick never blocks there).  Blocks are never returned
// to the system below kDescPoolBytes per device; beyond it, and when pinned memory runs out, a batch allocates and frees as before.
struct DescBlock {
    uint8_t *dev = nullptr, *host = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool recorded = false;         // `ev` has been recorded at least once since the block was (re)taken
    hipStream_t last = nullptr;    // the stream it was recorded on last
};
constexpr size_t kDescPoolBytes = (size_t)64 << 20;
struct DescPool { std::mutex mu; std::vector<DescBlock> free_blocks; size_t bytes = 0; };
// (never destroyed: freeing device memory from a static destructor would call into a runtime that may be gone already)
static DescPool &desc_pool(int device) { static DescPool *pools = new DescPool[16]; return pools[device & 15]; }
// (the device is current)
static bool desc_block_acquire(int device, size_t need, DescBlock *out) {
    DescPool &P = desc_pool(device);
    {
        std::lock_guard<std::mutex> lk(P.mu);
        size_t best = P.free_blocks.size();
        for (size_t i = 0; i < P.free_blocks.size(); i++)
            if (P.free_blocks[i].cap >= need && (best == P.free_blocks.size() || P.free_blocks[i].cap < P.free_blocks[best].cap)) best = i;
        if (best != P.free_blocks.size()) {
            *out = P.free_blocks[best];
            P.free_blocks.erase(P.free_blocks.begin() + (long)best);
            return true;
        }
        size_t cap = (size_t)64 << 10;
        while (cap < need) cap <<= 1;
        if (P.bytes + cap > kDescPoolBytes) return false;
        P.bytes += cap;
        need = cap;
    }
    DescBlock b;
    b.cap = need;
    hipError_t e = hipMalloc((void **)&b.dev, b.cap);
    if (e == hipSuccess) e = hipHostMalloc((void **)&b.host, b.cap, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&b.ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (b.dev) (void)hipFree(b.dev);
        if (b.host) (void)hipHostFree(b.host);
        std::lock_guard<std::mutex> lk(P.mu);
        P.bytes -= b.cap;
        return false;
    }
    *out = b;
    return true;
}
static void desc_block_release(int device, DescBlock &b) {
    if (!b.dev) return;
    DescPool &P = desc_pool(device);
    std::lock_guard<std::mutex> lk(P.mu);
    P.free_blocks.push_back(b);
    b = DescBlock{};
}

struct chv_batch {
    DescBlock blk;                 // pooled descriptors (d_ticks / d_layers / d_ticks2 point into blk.dev); blk.dev == nullptr: allocations of its own
    int device = 0;
    int n_ticks = 0, n_layers = 0;
    int target_format = 0;
    int maxW = 0, maxH = 0;
    int fast_path = -1;
    // a second launch that continues on the canvases (split_stream_prefix: the leading video layers through the streaming kernel, then the rest)
    int fast_path2 = -2;           // -2: none
    DTick *d_ticks2 = nullptr;
    std::vector<DTick> h_ticks2;
    DTick *d_ticks = nullptr;
    DLayer *d_layers = nullptr;
    std::vector<BatchDep> deps;    // distinct buffers the descriptors point into + the last upload waited for, per stream
    std::vector<DTick> h_ticks;    // host copies: launch geometry of the fast paths
    std::vector<DLayer> h_layers;
    std::string kernel_name;
    GeomCache geom;                // the strip kernels' per-layer geometry, computed once per launch configuration (geom_cache.h)
    // ---- chv_batch_rebind: what a picture slot (a tick's target: slot t; a layer's image: slot n_ticks + its index in h_layers) was created with ----
    struct SlotMeta { int32_t format, width, height, n_planes; };
    std::vector<SlotMeta> slot_meta;
    std::vector<chv_buffer *> slot_bufs;   // three per slot: the buffer behind every used plane (the descriptors hold raw addresses only) — `deps` follows them
    std::vector<uint32_t> slot_stamp;      // the rebind call that named the slot last (a slot named twice in one call is an error)
    uint32_t rebind_gen = 0;
    size_t lo = 0, t2o = 0, used = 0;      // a pooled block's sections: layers at `lo`, the second launch's ticks at `t2o`, `used` bytes in all
    // pinned lists of {offset, address} pairs for rebinds too long for kernel arguments, two of them in turn, and the event behind the last launch
    // that read each (index 2: behind the last whole-block copy out of the block's pinned twin)
    RebindItem *stage[2] = { nullptr, nullptr };
    RebindItem *stage_dev[2] = { nullptr, nullptr };
    size_t stage_cap[2] = { 0, 0 };
    hipEvent_t stage_ev[3] = { nullptr, nullptr, nullptr };
    bool stage_pending[3] = { false, false, false };
    int next_stage = 0;
    bool twin_rewritten = false;           // the twin has been refilled by a rebind (before that the copy that may still read it is the creation's: blk.ev)
};

static bool ctx_ok(chv_context *c) { return c && c->magic == 0x43485643 && c->stream; }
static bool buf_ok(const chv_buffer *b) { return b && b->magic == 0x43485642 && b->ptr; }

// ---------------------------------------------------------------------------
// devices
// ---------------------------------------------------------------------------
extern "C" int chv_device_count(int *count) {
    if (!count) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return hip_fail(e, "hipGetDeviceCount"); }
    *count = n;
    return CHV_OK;
}

extern "C" int chv_device_info_get(int device, chv_device_info *info) {
    if (!info) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    int n = 0;
    int rc = chv_device_count(&n);
    if (rc) return rc;
    if (device < 0 || device >= n) return fail(CHV_ERR_INVALID_DEVICE, "device %d of %d", device, n);
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    memset(info, 0, sizeof *info);
    info->index = device;
    info->device_type = 0;
    info->vendor_id = 0x1002;
    info->compute_units = p.multiProcessorCount;
    info->supports_images = 0;
    info->total_memory = p.totalGlobalMem;
    snprintf(info->name, sizeof info->name, "%s", p.name);
    snprintf(info->arch, sizeof info->arch, "%s", p.gcnArchName);
    // kernels in this library are built for gfx950 only
    info->available = strncmp(p.gcnArchName, "gfx950", 6) == 0;
    return CHV_OK;
}

// ---------------------------------------------------------------------------
// contexts
// ---------------------------------------------------------------------------
static int context_new(int device, std::shared_ptr<DeviceShared> shared, chv_context **out) {
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<chv_context> c(new chv_context);
    c->device = device;
    c->shared = std::move(shared);
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    hipError_t e = hipHostMalloc((void **)&c->desc_host, kDescSlots * kDescSlotBytes, hipHostMallocMapped);
    if (e != hipSuccess) { (void)hipStreamDestroy(c->stream); return hip_fail(e, "hipHostMalloc(descriptors)"); }
    e = hipMalloc((void **)&c->desc_dev, kDescSlots * kDescSlotBytes);
    if (e != hipSuccess) { (void)hipHostFree(c->desc_host); (void)hipStreamDestroy(c->stream); return hip_fail(e, "hipMalloc(descriptors)"); }
    *out = c.release();
    return CHV_OK;
}

extern "C" int chv_context_create(int device, chv_context **out) {
    if (!out) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    *out = nullptr;
    chv_device_info info;
    int rc = chv_device_info_get(device, &info);
    if (rc) return rc;
    if (!info.available)
        return fail(CHV_ERR_DEVICE_NOT_AVAILABLE, "device %d is %s; this library carries gfx950 code only", device, info.arch);
    auto shared = std::make_shared<DeviceShared>();
    shared->device = device;
    return context_new(device, shared, out);
}

extern "C" int chv_context_share(chv_context *parent, chv_context **out) {
    if (!out) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    *out = nullptr;
    if (!ctx_ok(parent)) return fail(CHV_ERR_INVALID_CONTEXT, "bad parent context");
    int rc = context_new(parent->device, parent->shared, out);
    if (rc == CHV_OK) (*out)->library = parent->library;      // ComputeContext(other:) copies the library, compute.cl.swift:82-87
    return rc;
}

extern "C" int chv_context_destroy(chv_context *c) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    (void)hipSetDevice(c->device);
    (void)flush_pending(c);             // (a pass left open: its kernels were accepted, they run)
    (void)hipStreamSynchronize(c->stream);
    for (auto &s : c->staging) {
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.host) (void)hipHostFree(s.host);
    }
    for (auto &d : c->desc_group) if (d.done) (void)hipEventDestroy(d.done);
    if (c->desc_host) (void)hipHostFree(c->desc_host);
    if (c->desc_dev) (void)hipFree(c->desc_dev);
    (void)hipStreamDestroy(c->stream);
    c->magic = 0;
    c->stream = nullptr;
    delete c;
    return CHV_OK;
}

extern "C" int chv_context_device(chv_context *c, int *device) {
    if (!ctx_ok(c) || !device) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    *device = c->device;
    return CHV_OK;
}
// NUMA node of the device's PCIe root (sysfs), -1 when the platform does not say: a host that pins its upload ring on that
// node (first touch from a thread bound there) keeps H2D copies off the inter-socket link
extern "C" int chv_context_numa_node(chv_context *c, int *node) {
    if (!ctx_ok(c) || !node) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    *node = -1;
    char bus[64] = { 0 };
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, c->device) != hipSuccess) { (void)hipGetLastError(); return CHV_OK; }
    for (char *p = bus; *p; p++) *p = (char)tolower((unsigned char)*p);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    if (FILE *f = fopen(path.c_str(), "r")) {
        int n = -1;
        if (fscanf(f, "%d", &n) == 1) *node = n;
        fclose(f);
    }
    return CHV_OK;
}
extern "C" int chv_context_stream(chv_context *c, void **s) {
    if (!ctx_ok(c) || !s) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);       // (whoever asks for the stream is about to put work behind what the pass holds)
    *s = (void *)c->stream;
    return CHV_OK;
}

// ---------------------------------------------------------------------------
// buffers and transfers
// ---------------------------------------------------------------------------
extern "C" int chv_buffer_alloc(chv_context *c, size_t bytes, chv_buffer **out) {
    if (!out) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    *out = nullptr;
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (bytes == 0) return fail(CHV_ERR_INVALID_VALUE, "zero-sized buffer");
    HIP_TRY(hipSetDevice(c->device));
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    chv_buffer *b = new chv_buffer;
    b->ptr = p; b->size = bytes; b->device = c->device; b->owned = true;
    *out = b;
    return CHV_OK;
}

extern "C" int chv_buffer_wrap(chv_context *c, void *device_ptr, size_t bytes, chv_buffer **out) {
    if (!out) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    *out = nullptr;
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (!device_ptr || bytes == 0) return fail(CHV_ERR_INVALID_VALUE, "null/empty device memory");
    chv_buffer *b = new chv_buffer;
    b->ptr = device_ptr; b->size = bytes; b->device = c->device; b->owned = false;
    *out = b;
    return CHV_OK;
}

static int buffer_free_now(chv_buffer *b);
extern "C" int chv_buffer_free(chv_buffer *b) {
    if (!b || b->magic != 0x43485642) return fail(CHV_ERR_INVALID_VALUE, "bad buffer");
    {
        std::lock_guard<std::mutex> lock(g_pin_mu);
        if (b->doomed) return fail(CHV_ERR_INVALID_VALUE, "buffer freed twice");
        if (b->pins > 0) { b->doomed = true; return CHV_OK; }      // a pending pass still names it: freed when that pass has been launched
    }
    return buffer_free_now(b);
}
static int buffer_free_now(chv_buffer *b) {
    if (b->owned && b->ptr) {
        // any thread, any time: make the owning device current first
        // (compute.cuda.swift:82-88 pushes the context in deinit for the same reason)
        (void)hipSetDevice(b->device);
        (void)hipFree(b->ptr);  // hipFree waits for in-flight work on the allocation
    }
    if (b->ready) { (void)hipSetDevice(b->device); (void)hipEventDestroy(b->ready); b->ready = nullptr; }
    b->magic = 0;
    b->ptr = nullptr;
    delete b;
    return CHV_OK;
}

extern "C" int chv_buffer_info(chv_buffer *b, void **device_ptr, size_t *bytes) {
    if (!buf_ok(b)) return fail(CHV_ERR_INVALID_VALUE, "bad buffer");
    if (device_ptr) *device_ptr = b->ptr;
    if (bytes) *bytes = b->size;
    return CHV_OK;
}

extern "C" int chv_plane_alloc(chv_context *c, int width, int height, int components,
                               chv_buffer **out, size_t *pitch) {
    if (!out || !pitch) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    if (width <= 0 || height <= 0) return fail(CHV_ERR_INVALID_OPERATION, "plane size %dx%d", width, height);
    if (components != 1 && components != 2 && components != 4)
        return fail(CHV_ERR_BAD_INPUT, "components must be 1, 2 or 4, got %d", components);
    // rows start on a 128-byte cache line; widths that already are a multiple of 128 bytes stay packed,
    // so a packed host plane of the same stride uploads as one linear copy
    size_t row = (size_t)width * components;
    size_t p = (row + 127) & ~(size_t)127;
    *pitch = p;
    return chv_buffer_alloc(c, p * (size_t)height, out);
}

static int check_span(const chv_buffer *b, size_t offset, size_t pitch, size_t width_bytes, size_t rows,
                      const char *what) {
    if (!buf_ok(b)) return fail(CHV_ERR_BAD_INPUT, "%s: bad buffer", what);
    if (rows == 0 || width_bytes == 0) return fail(CHV_ERR_INVALID_VALUE, "%s: empty region", what);
    if (pitch < width_bytes) return fail(CHV_ERR_BAD_INPUT, "%s: pitch %zu < row bytes %zu", what, pitch, width_bytes);
    size_t end = 0, total = 0;
    if (__builtin_mul_overflow(rows - 1, pitch, &end) || __builtin_add_overflow(end, width_bytes, &end) ||
        __builtin_add_overflow(end, offset, &end) || __builtin_mul_overflow(rows, width_bytes, &total))
        return fail(CHV_ERR_BAD_INPUT, "%s: region size overflows", what);
    if (end > b->size) return fail(CHV_ERR_BAD_INPUT, "%s: region ends at %zu, buffer has %zu bytes", what, end, b->size);
    return CHV_OK;
}

extern "C" int chv_upload(chv_context *c, chv_buffer *dst, size_t dst_offset, size_t dst_pitch,
                          const void *src, size_t src_pitch, size_t width_bytes, size_t rows, int async) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (!src) return fail(CHV_ERR_BAD_INPUT, "null source");
    int rc = check_span(dst, dst_offset, dst_pitch, width_bytes, rows, "upload");
    if (rc) return rc;
    if (src_pitch < width_bytes) return fail(CHV_ERR_BAD_INPUT, "source pitch %zu < row bytes %zu", src_pitch, width_bytes);
    HIP_TRY(hipSetDevice(c->device));
    uint8_t *d = (uint8_t *)dst->ptr + dst_offset;
    auto copy_h2d = [&](const void *from, size_t from_pitch) -> hipError_t {
        // one contiguous block on both sides -> a linear copy
        if (dst_pitch == width_bytes && from_pitch == width_bytes) return hipMemcpyAsync(d, from, width_bytes * rows, hipMemcpyHostToDevice, c->stream);
        return hipMemcpy2DAsync(d, dst_pitch, from, from_pitch, width_bytes, rows, hipMemcpyHostToDevice, c->stream);
    };
    // an earlier asynchronous upload into the same buffer from another context must land first (stream order
    // only covers this context's own copies)
    rc = wait_for_buffer(dst, c->stream);
    if (rc) return rc;
    if (!async) {
        HIP_TRY(copy_h2d(src, src_pitch));
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::lock_guard<std::mutex> lock(dst->mu);
        dst->ready_stream = nullptr;   // complete: nobody has to wait
        return CHV_OK;
    }
    if (async == 2) {
        // caller-owned pinned memory (chv_host_alloc): no staging copy
        HIP_TRY(copy_h2d(src, src_pitch));
        return mark_uploaded(dst, c->stream);
    }
    // stage into pinned memory so the caller's bytes are only borrowed for this call
    StagingSlot &s = c->staging[c->next_staging];
    c->next_staging = (c->next_staging + 1) % kStagingSlots;
    if (s.pending) { HIP_TRY(hipEventSynchronize(s.done)); s.pending = false; }
    size_t need = width_bytes * rows;
    if (s.cap < need) {
        if (s.host) { HIP_TRY(hipHostFree(s.host)); s.host = nullptr; s.cap = 0; }
        size_t cap = (need + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);   // need = rows * width_bytes, overflow-checked by check_span
        HIP_TRY(hipHostMalloc(&s.host, cap, hipHostMallocDefault));
        s.cap = cap;
    }
    if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    const uint8_t *sp = (const uint8_t *)src;
    uint8_t *hp = (uint8_t *)s.host;
    if (src_pitch == width_bytes) memcpy(hp, sp, need);
    else for (size_t r = 0; r < rows; r++) memcpy(hp + r * width_bytes, sp + r * src_pitch, width_bytes);
    HIP_TRY(copy_h2d(hp, width_bytes));
    HIP_TRY(hipEventRecord(s.done, c->stream));
    s.pending = true;
    return mark_uploaded(dst, c->stream);
}

static int mark_uploaded(chv_buffer *b, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(b->mu);
    if (!b->ready) HIP_TRY(hipEventCreateWithFlags(&b->ready, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(b->ready, stream));
    b->ready_stream = stream;
    b->ready_seq++;
    return CHV_OK;
}

static int wait_for_buffer(chv_buffer *b, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(b->mu);
    if (!b->ready_stream) return CHV_OK;
    if (hipEventQuery(b->ready) == hipSuccess) { b->ready_stream = nullptr; return CHV_OK; }   // landed: nobody has to wait any more
    (void)hipGetLastError();                                                                    // hipErrorNotReady is not an error here
    if (b->ready_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, b->ready, 0));
    return CHV_OK;
}

extern "C" int chv_host_alloc(chv_context *c, size_t bytes, void **out) {
    if (!out) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    *out = nullptr;
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (bytes == 0) return fail(CHV_ERR_INVALID_VALUE, "zero-sized allocation");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return CHV_OK;
}

extern "C" int chv_host_free(chv_context *c, void *ptr) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (!ptr) return fail(CHV_ERR_INVALID_VALUE, "null pointer");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostFree(ptr));
    return CHV_OK;
}

static int download_enqueue(chv_context *c, void *dst, size_t dst_pitch, chv_buffer *src,
                            size_t src_offset, size_t src_pitch, size_t width_bytes, size_t rows) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (!dst) return fail(CHV_ERR_BAD_INPUT, "null destination");
    int rc = check_span(src, src_offset, src_pitch, width_bytes, rows, "download");
    if (rc) return rc;
    if (dst_pitch < width_bytes) return fail(CHV_ERR_BAD_INPUT, "destination pitch %zu < row bytes %zu", dst_pitch, width_bytes);
    HIP_TRY(hipSetDevice(c->device));
    // a picture uploaded asynchronously on another context (GPUBarrierUpload's) and read back through this one
    // (GPUBarrierDownload's, compute.swift:175-255): order the read behind the upload
    rc = wait_for_buffer(src, c->stream);
    if (rc) return rc;
    const uint8_t *from = (const uint8_t *)src->ptr + src_offset;
    // one contiguous block on both sides -> a linear copy (a slab of frames: the link gives its full rate to copies of 8 MB and more)
    if (dst_pitch == width_bytes && src_pitch == width_bytes) HIP_TRY(hipMemcpyAsync(dst, from, width_bytes * rows, hipMemcpyDeviceToHost, c->stream));
    else HIP_TRY(hipMemcpy2DAsync(dst, dst_pitch, from, src_pitch, width_bytes, rows, hipMemcpyDeviceToHost, c->stream));
    return CHV_OK;
}

extern "C" int chv_download(chv_context *c, void *dst, size_t dst_pitch, chv_buffer *src,
                            size_t src_offset, size_t src_pitch, size_t width_bytes, size_t rows) {
    int rc = download_enqueue(c, dst, dst_pitch, src, src_offset, src_pitch, width_bytes, rows);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CHV_OK;
}

// The copy is ordered on the context's stream and the call returns at once: `dst` is pinned memory (chv_host_alloc) whose bytes are the
// picture's once the stream has passed the copy — chv_event_record + chv_event_synchronize, or chv_pass_end(wait) on this context.  Work of
// OTHER contexts that writes `src` (the mixer's tick) is ordered in front of it with chv_event_record there and chv_event_wait here, as
// between any two contexts: a download barrier running on a context of its own (GPUBarrierDownload, compute.swift:217-255) then overlaps the
// D2H copy of tick t with the kernels of tick t + 1.
// `dst` must be pinned (chv_host_alloc, or memory the caller registered with the runtime): into pageable memory the runtime stages the copy and
// blocks the host, and "valid once the stream has passed the copy" holds only loosely — such a destination gets the synchronous path instead
// (the bytes are there when the call returns; nothing the caller does afterwards can be wrong).
static bool host_range_is_pinned(const void *p, size_t bytes) {
    if (!p || bytes == 0) return false;
    for (const uint8_t *q : { (const uint8_t *)p, (const uint8_t *)p + bytes - 1 }) {
        hipPointerAttribute_t a;
        memset(&a, 0, sizeof a);
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (a.type != hipMemoryTypeHost) return false;
    }
    return true;
}
extern "C" int chv_download_async(chv_context *c, void *dst, size_t dst_pitch, chv_buffer *src,
                                  size_t src_offset, size_t src_pitch, size_t width_bytes, size_t rows) {
    int rc = download_enqueue(c, dst, dst_pitch, src, src_offset, src_pitch, width_bytes, rows);
    if (rc) return rc;
    if (rows && width_bytes && !host_range_is_pinned(dst, (rows - 1) * dst_pitch + width_bytes)) HIP_TRY(hipStreamSynchronize(c->stream));
    return CHV_OK;
}

// ---------------------------------------------------------------------------
// descriptor building
// ---------------------------------------------------------------------------
struct KernelShape {
    int src_planes;      // 0 for clear
    int src_comps[3];
    int target_format;   // TargetFormat
    int kind;            // LayerKind
    int swizzle;
    bool is_clear;
};

static int kernel_shape(int kernel, KernelShape *s) {
    memset(s, 0, sizeof *s);
    auto yuv_nv12 = [&](int tf, int kind) { s->src_planes = 2; s->src_comps[0] = 1; s->src_comps[1] = 2; s->target_format = tf; s->kind = kind; };
    auto yuv_420p = [&](int tf, int kind) { s->src_planes = 3; s->src_comps[0] = s->src_comps[1] = s->src_comps[2] = 1; s->target_format = tf; s->kind = kind; };
    auto rgb = [&](int tf, int kind, int swz) { s->src_planes = 1; s->src_comps[0] = 4; s->target_format = tf; s->kind = kind; s->swizzle = swz; };
    switch (kernel) {
    case CHV_K_IMG_NV12_NV12: yuv_nv12(TF_NV12, LK_YUV_FROM_NV12); break;
    case CHV_K_IMG_Y420P_NV12: yuv_420p(TF_NV12, LK_YUV_FROM_Y420P); break;
    case CHV_K_IMG_Y420P_Y420P: yuv_420p(TF_Y420P, LK_YUV_FROM_Y420P); break;
    case CHV_K_IMG_BGRA_NV12: rgb(TF_NV12, LK_YUV_FROM_RGB, 1); break;   // .zyxw, kernels.cl.swift:518
    case CHV_K_IMG_RGBA_NV12: rgb(TF_NV12, LK_YUV_FROM_RGB, 0); break;
    case CHV_K_IMG_BGRA_Y420P: rgb(TF_Y420P, LK_YUV_FROM_RGB, 1); break;
    case CHV_K_IMG_RGBA_Y420P: rgb(TF_Y420P, LK_YUV_FROM_RGB, 0); break;
    case CHV_K_IMG_BGRA_BGRA: rgb(TF_BGRA, LK_BGRA_METAL, 0); break;
    case CHV_K_IMG_NV12_BGRA: yuv_nv12(TF_BGRA, LK_BGRA_FROM_NV12); break;
    case CHV_K_IMG_Y420P_BGRA: yuv_420p(TF_BGRA, LK_BGRA_FROM_Y420P); break;
    case CHV_K_IMG_BGRA_BGRA_TX: rgb(TF_BGRA, LK_BGRA_FROM_RGB, 0); break;
    case CHV_K_IMG_RGBA_BGRA_TX: rgb(TF_BGRA, LK_BGRA_FROM_RGB, 1); break;
    case CHV_K_IMG_BGRA_NV12_INT: rgb(TF_NV12, LK_YUV_FROM_RGB_INT, 1); break;
    case CHV_K_IMG_RGBA_NV12_INT: rgb(TF_NV12, LK_YUV_FROM_RGB_INT, 0); break;
    case CHV_K_IMG_BGRA_Y420P_INT: rgb(TF_Y420P, LK_YUV_FROM_RGB_INT, 1); break;
    case CHV_K_IMG_RGBA_Y420P_INT: rgb(TF_Y420P, LK_YUV_FROM_RGB_INT, 0); break;
    case CHV_K_IMG_CLEAR_NV12: s->is_clear = true; s->target_format = TF_NV12; break;
    case CHV_K_IMG_CLEAR_Y420P: s->is_clear = true; s->target_format = TF_Y420P; break;
    case CHV_K_IMG_CLEAR_BGRA: case CHV_K_IMG_CLEAR_RGBA: s->is_clear = true; s->target_format = TF_BGRA; break;
    case CHV_K_IMG_CLEAR_YUVS:
        // an enum case for which no backend of the reference has a kernel either
        return fail(CHV_ERR_KERNEL_NOT_FOUND, "kernel %s has no implementation", chv_kernel_name(kernel));
    case CHV_K_SND_S16I_S16I: case CHV_K_ME_FULLSEARCH:
        // (not layer kernels: chv_run_kernel runs them directly, run_idle_kernel)
        return fail(CHV_ERR_INVALID_OPERATION, "%s is not a picture-layer kernel: issue it through chv_run_kernel", chv_kernel_name(kernel));
    default:
        return fail(CHV_ERR_KERNEL_NOT_FOUND, "unknown kernel id %d", kernel);
    }
    return CHV_OK;
}

// buffers referenced by the descriptors being built (for upload -> kernel ordering)
static thread_local std::vector<chv_buffer *> *g_deps = nullptr;

struct DepScope {
    std::vector<chv_buffer *> bufs;
    DepScope() { g_deps = &bufs; }
    ~DepScope() { g_deps = nullptr; }
    // distinct buffers (a picture's planes usually share one allocation)
    std::vector<BatchDep> deps() const {
        // (a 256-tick batch names 2 300 planes of some hundreds of buffers, and is built afresh for every group tick of a host that batches: the
        // quadratic walk this replaces was 130 of the 300 us chv_batch_create took for it, tools/batch_create_probe.cpp.  A picture's planes
        // share an allocation — consecutive repeats go first —, the rest through a small open-addressing set.)
        std::vector<BatchDep> out;
        const size_t n = bufs.size();
        if (n <= 24) {
            for (chv_buffer *b : bufs) {
                bool seen = false;
                for (const BatchDep &d : out) seen = seen || d.buf == b;
                if (!seen) out.push_back(BatchDep{ b, nullptr, 0 });
            }
            return out;
        }
        size_t cap = 64;
        while (cap < 2 * n) cap <<= 1;
        std::vector<chv_buffer *> tab(cap, nullptr);
        chv_buffer *last = nullptr;
        for (chv_buffer *b : bufs) {
            if (b == last) continue;
            last = b;
            size_t h = (size_t)(((uintptr_t)b >> 6) * 0x9E3779B97F4A7C15ull >> 32) & (cap - 1);
            while (tab[h] && tab[h] != b) h = (h + 1) & (cap - 1);
            if (!tab[h]) { tab[h] = b; out.push_back(BatchDep{ b, nullptr, 0 }); }
        }
        return out;
    }
};

// Make `stream` wait for pending asynchronous uploads into the buffers a launch reads.  A batch remembers, per buffer,
// the (stream, upload) it last waited for, so replaying it on the same stream with no new upload costs nothing; a
// different stream, or a newer upload, waits again.
static int wait_for_uploads(hipStream_t stream, std::vector<BatchDep> &deps) {
    for (BatchDep &d : deps) {
        chv_buffer *b = d.buf;
        if (!b->ready_stream.load(std::memory_order_acquire)) continue;          // nothing pending (a batch of 256 mixers names a thousand buffers)
        std::lock_guard<std::mutex> lock(b->mu);
        if (!b->ready_stream || b->ready_stream == stream) continue;
        if (d.stream == stream && d.seq == b->ready_seq) continue;
        if (hipEventQuery(b->ready) == hipSuccess) { b->ready_stream = nullptr; continue; }
        (void)hipGetLastError();
        HIP_TRY(hipStreamWaitEvent(stream, b->ready, 0));
        d.stream = stream; d.seq = b->ready_seq;
    }
    return CHV_OK;
}

// align: what the plane's start address and pitch must be a multiple of; 0: the rule of every 8-bit format (4 for a 4-component plane)
static int plane_to_device(const chv_plane &p, int comps, int device, DPlane *out, int err, const char *what, int idx, int align = 0) {
    if (!buf_ok(p.buffer)) return fail(err, "%s plane %d: no device buffer", what, idx);
    if (p.buffer->device != device) return fail(err, "%s plane %d lives on device %d, context on %d", what, idx, p.buffer->device, device);
    if (p.width <= 0 || p.height <= 0) return fail(err, "%s plane %d: size %dx%d", what, idx, p.width, p.height);
    if (p.components != comps) return fail(err, "%s plane %d: %d components, kernel expects %d", what, idx, p.components, comps);
    const int64_t row_bytes = (int64_t)p.width * comps;
    if (row_bytes > 0x3fffffff || p.height > 0x3fffffff) return fail(err, "%s plane %d: size %dx%d is out of range", what, idx, p.width, p.height);
    if ((int64_t)p.pitch < row_bytes) return fail(err, "%s plane %d: pitch %d < %lld", what, idx, p.pitch, (long long)row_bytes);
    size_t end = 0;
    if (__builtin_mul_overflow((size_t)(p.height - 1), (size_t)p.pitch, &end) || __builtin_add_overflow(end, (size_t)row_bytes, &end) ||
        __builtin_add_overflow(end, p.offset, &end))
        return fail(err, "%s plane %d: extent overflows", what, idx);
    if (end > p.buffer->size) return fail(err, "%s plane %d: extent %zu exceeds buffer size %zu", what, idx, end, p.buffer->size);
    if (!align && comps == 4 && (((uintptr_t)p.buffer->ptr + p.offset) & 3 || (p.pitch & 3)))
        return fail(err, "%s plane %d: 4-component planes must be 4-byte aligned", what, idx);
    if (align && ((((uintptr_t)p.buffer->ptr + p.offset) | (uintptr_t)p.pitch) & (uintptr_t)(align - 1)))
        return fail(err, "%s plane %d: start and pitch must be multiples of %d", what, idx, align);
    out->ptr = (uint8_t *)p.buffer->ptr + p.offset;
    out->w = p.width; out->h = p.height; out->pitch = p.pitch; out->comps = comps;
    if (g_deps) g_deps->push_back(p.buffer);
    return CHV_OK;
}

// do two planes (both accepted by plane_to_device) share device memory?  A plane spans ptr + offset .. + (height - 1) * pitch + row bytes;
// two handles over one piece of memory (chv_buffer_wrap) and views with plane offsets are compared by what they address
static bool planes_overlap(const chv_plane &a, const chv_plane &b) {
    if (!buf_ok(a.buffer) || !buf_ok(b.buffer) || a.buffer->device != b.buffer->device) return false;
    if (a.width <= 0 || a.height <= 0 || b.width <= 0 || b.height <= 0) return false;
    const uintptr_t a0 = (uintptr_t)a.buffer->ptr + a.offset, b0 = (uintptr_t)b.buffer->ptr + b.offset;
    const uintptr_t a1 = a0 + (size_t)(a.height - 1) * a.pitch + (size_t)a.width * a.components;
    const uintptr_t b1 = b0 + (size_t)(b.height - 1) * b.pitch + (size_t)b.width * b.components;
    return a0 < b1 && b0 < a1;
}

static int target_to_device(const chv_image *t, int target_format, int device, DImage *out) {
    if (!t) return fail(CHV_ERR_BAD_TARGET, "null target");
    static const int np[3] = { 2, 3, 1 };
    static const int comps[3][3] = { { 1, 2, 0 }, { 1, 1, 1 }, { 4, 0, 0 } };
    if (t->n_planes != np[target_format])
        return fail(CHV_ERR_BAD_TARGET, "target has %d planes, kernel writes %d", t->n_planes, np[target_format]);
    memset(out, 0, sizeof *out);
    for (int i = 0; i < t->n_planes; i++) {
        int rc = plane_to_device(t->planes[i], comps[target_format][i], device, &out->pl[i], CHV_ERR_BAD_TARGET, "target", i);
        if (rc) return rc;
    }
    return CHV_OK;
}

// host-side analysis of a layer's uniforms for fast-path selection
static int32_t layer_flags(const float *u) {
    int32_t f = 0;
    auto axis = [&](const float *m) {
        // row 0 must not depend on y/z, row 1 not on x/z, rows 2,3 = (0,0,*,*), so that
        // component 0 is a function of x only and component 1 of y only
        return m[1] == 0.f && m[2] == 0.f && m[4] == 0.f && m[6] == 0.f;
    };
    const float *T = u + U_TRANSFORM, *X = u + U_TEXTURE, *B = u + U_BORDER;
    // uv = textureTx . tx uses all four tx components: tx.z/tx.w must not depend on x or y
    bool tzw_const = T[8] == 0.f && T[9] == 0.f && T[12] == 0.f && T[13] == 0.f;
    if (axis(T) && axis(B) && axis(X) && tzw_const) f |= LF_AXIS_ALIGNED;
    // no fill contribution: alpha is exactly zero AND the colour is finite (0 * inf would be NaN)
    // (checked on fill * 255, the code-scale value the BGRA-target family multiplies by the alpha)
    auto finite255 = [](float c) { float v = c * 255.0f; return v - v == 0.f; };
    bool fill_finite = finite255(u[U_FILL]) && finite255(u[U_FILL + 1]) && finite255(u[U_FILL + 2]);
    if (u[U_OPACITY] * u[U_FILL + 3] == 0.f && fill_finite) f |= LF_NO_FILL;
    if (u[U_OPACITY] == 1.f) f |= LF_OPAQUE;
    // bounded matrices: with |entry| < 2^60 and |nx|, |ny| <= 3 no product of the geometry prologue overflows, so the
    // zero entries of an axis-aligned layer contribute exact zeros (geometry_axis, pixel_math.hip.h)
    bool bounded = true;
    for (int i = 0; i < 48; i++) bounded = bounded && std::fabs(u[i]) < 0x1p60f;      // false for NaN as well
    if (bounded) f |= LF_BOUNDED;
    return f;
}

// Conservative bounding box of {pixels whose border coordinates lie in [0,1]^2}.  Axis-aligned
// layers only (border.x depends on x alone); everything else gets the whole canvas.  The box is
// computed in double with a 2-pixel margin, far more than the float evaluation can differ by.
static void layer_bbox(DLayer *L, int W, int H) {
    L->bbox[0] = 0; L->bbox[1] = 0; L->bbox[2] = W; L->bbox[3] = H;
    const float *B = L->u + U_BORDER;
    if (!(L->flags & LF_AXIS_ALIGNED)) {
        // Rotated / sheared layers: the border coordinates are affine in the pixel — b = A n + t with n = (2 x / W - 1, 2 y / H - 1), z = 0, w = 1
        // (geometry(), pixel_math.hip.h) — so the pixels a layer can touch lie in the parallelogram A^-1 ([0,1]^2 - t).  Its box, in double with the
        // same 2-pixel margin; entries large enough for the float evaluation to differ by more than that (or a singular A) keep the whole canvas.
        // (Until round 4 these layers had the whole canvas for a box: a rotated logo made EVERY strip of the tick run its per-pixel loop.)
        const double a = B[0], b = B[1], c = B[4], d = B[5], tx = B[3], ty = B[7];
        double big = 0.0;
        for (double v : { a, b, c, d, tx, ty }) { if (!(v - v == 0.0)) return; big = std::max(big, std::fabs(v)); }
        const double det = a * d - b * c;
        if (!(big < 1048576.0) || !(std::fabs(det) > 1e-9 * std::max(1.0, big * big))) return;
        // The device evaluates b = A n + t in float (error ~ 4e-7 big) and the box is the image of [0,1]^2 under A^-1, which amplifies that by
        // ~ big / |det|: the float-accepted pixels can stick out of the double parallelogram by ~ 8e-7 big^2 / |det| * W / 2 pixels — more than
        // the 2-pixel margin once big^2 / |det| passes a few thousand (thin or strongly sheared layers with a large translation term).  Those keep
        // the whole canvas, as every such layer did before round 4.
        if (!(big * big / std::fabs(det) < 1e3)) return;
        double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
        for (int k = 0; k < 4; k++) {
            const double u = (k & 1) - tx, v = (k >> 1) - ty;
            const double nx = (d * u - b * v) / det, ny = (-c * u + a * v) / det;
            const double px = (nx + 1.0) * W / 2.0, py = (ny + 1.0) * H / 2.0;
            x0 = std::min(x0, px); x1 = std::max(x1, px); y0 = std::min(y0, py); y1 = std::max(y1, py);
        }
        if (!(x0 - x0 == 0.0 && x1 - x1 == 0.0 && y0 - y0 == 0.0 && y1 - y1 == 0.0)) return;
        auto clampi = [](double v, int n) { return (int32_t)std::min(std::max(v, 0.0), (double)n); };
        L->bbox[0] = clampi(std::floor(x0) - 2.0, W); L->bbox[2] = clampi(std::ceil(x1) + 3.0, W);
        L->bbox[1] = clampi(std::floor(y0) - 2.0, H); L->bbox[3] = clampi(std::ceil(y1) + 3.0, H);
        return;
    }
    auto range = [](double k, double c, int n, int32_t *lo, int32_t *hi) {
        // 0 <= k * (2*x/n - 1) + c <= 1
        if (!(k - k == 0.0) || !(c - c == 0.0)) return;
        if (k == 0.0) { if (c < -1e-3 || c > 1.0 + 1e-3) { *lo = 0; *hi = 0; } return; }
        double a = ((0.0 - c) / k + 1.0) * n / 2.0, b = ((1.0 - c) / k + 1.0) * n / 2.0;
        if (a > b) std::swap(a, b);
        double l = std::floor(a) - 2.0, h = std::ceil(b) + 3.0;
        *lo = (int32_t)std::min(std::max(l, 0.0), (double)n);
        *hi = (int32_t)std::min(std::max(h, 0.0), (double)n);
    };
    // row 0: b0 = nx*B[0] + (ny*B[1] + 0*B[2]) + B[3] with B[1] = B[2] = 0
    range((double)B[0], (double)B[3], W, &L->bbox[0], &L->bbox[2]);
    range((double)B[5], (double)B[7], H, &L->bbox[1], &L->bbox[3]);
}

// LF_COVERS + ibox (device_types.h): the canvas pixels an opaque YUV-source layer replaces for sure — where border, transform and texture
// coordinates all lie in [0, 1] — shrunk by two pixels per side (the same margin layer_bbox adds).  Axis-aligned, bounded layers on BGRA canvases.
static void layer_inner_box(DLayer *L, int W, int H, int target_format) {
    L->ibox[0] = L->ibox[1] = L->ibox[2] = L->ibox[3] = 0;
    L->flags &= ~LF_COVERS;
    const int need = LF_AXIS_ALIGNED | LF_BOUNDED | LF_OPAQUE;
    if (target_format != TF_BGRA || (L->flags & need) != need) return;
    if (L->kind != LK_BGRA_FROM_NV12 && L->kind != LK_BGRA_FROM_Y420P) return;          // (RGB sources carry per-pixel alpha)
    const float *T = L->u + U_TRANSFORM, *X = L->u + U_TEXTURE, *B = L->u + U_BORDER;
    // per axis: v(n) = k n + c in [0, 1] for the three coordinates; n = 2 p / size - 1
    auto inner = [](double k, double c, int n, double *lo, double *hi) {
        if (!(k - k == 0.0) || !(c - c == 0.0) || k == 0.0) { *lo = 1.0; *hi = 0.0; return; }
        double a = ((0.0 - c) / k + 1.0) * n / 2.0, b = ((1.0 - c) / k + 1.0) * n / 2.0;
        if (a > b) std::swap(a, b);
        *lo = std::max(*lo, std::ceil(a) + 2.0); *hi = std::min(*hi, std::floor(b) - 2.0);
    };
    const double t3 = T[15];
    // The device evaluates u = fl(fl(t0 X0) + fl(t3 X3)) in float; with large, mutually cancelling terms its error can exceed the 2-pixel
    // shrink, and a strip judged covered would drop the layers beneath pixels that are in fact outside the texture range.  Modest magnitudes only
    // (the animator's matrices are O(canvas / picture): single digits to a few hundred).
    for (double m : { (double)T[3] * X[0], t3 * X[3], (double)T[7] * X[5], t3 * X[7], (double)T[3], (double)T[7], (double)B[3], (double)B[7],
                      (double)T[0] * X[0], (double)T[5] * X[5], (double)B[0], (double)B[5] })
        if (!(std::fabs(m) < 1e3)) return;
    double xl = 0.0, xh = W, yl = 0.0, yh = H;
    inner(B[0], B[3], W, &xl, &xh); inner(T[0], T[3], W, &xl, &xh); inner((double)T[0] * X[0], (double)T[3] * X[0] + t3 * X[3], W, &xl, &xh);
    inner(B[5], B[7], H, &yl, &yh); inner(T[5], T[7], H, &yl, &yh); inner((double)T[5] * X[5], (double)T[7] * X[5] + t3 * X[7], H, &yl, &yh);
    if (!(xl < xh && yl < yh)) return;
    L->ibox[0] = (int32_t)xl; L->ibox[2] = (int32_t)xh; L->ibox[1] = (int32_t)yl; L->ibox[3] = (int32_t)yh;
    L->flags |= LF_COVERS;
}

static int layer_to_device(const chv_layer &l, int device, int *target_format, DLayer *out) {
    KernelShape s;
    int rc = kernel_shape(l.kernel, &s);
    if (rc) return rc;
    if (s.is_clear) return fail(CHV_ERR_INVALID_OPERATION, "%s is not a layer kernel", chv_kernel_name(l.kernel));
    if (*target_format < 0) *target_format = s.target_format;
    else if (*target_format != s.target_format)
        return fail(CHV_ERR_BAD_TARGET, "%s does not write this target format", chv_kernel_name(l.kernel));
    if (l.image.n_planes < s.src_planes)
        return fail(CHV_ERR_BAD_INPUT, "%s needs %d input planes, image has %d", chv_kernel_name(l.kernel), s.src_planes, l.image.n_planes);
    memset(out, 0, sizeof *out);
    for (int i = 0; i < s.src_planes; i++) {
        rc = plane_to_device(l.image.planes[i], s.src_comps[i], device, &out->src.pl[i], CHV_ERR_BAD_INPUT, "input", i);
        if (rc) return rc;
    }
    static_assert(sizeof(chv_uniforms) == 236, "ImageUniforms must be 236 bytes (compute.swift:76-86)");
    memcpy(out->u, &l.uniforms, sizeof(chv_uniforms));
    if (s.kind == LK_BGRA_METAL) {
        if (!(out->u[U_OUTSIZE] > 0.f) || !(out->u[U_OUTSIZE + 1] > 0.f))
            return fail(CHV_ERR_INVALID_VALUE, "img_bgra_bgra needs a positive outputSize in the uniforms");
    }
    out->kind = s.kind;
    out->swizzle = s.swizzle;
    out->csc = l.opts.colorspace & 3;
    out->flags = layer_flags(out->u);
    return CHV_OK;
}

static int tick_to_device(const chv_tick &t, int device, int forced_target_format, DTick *dt,
                          std::vector<DLayer> *layers, int *target_format_out) {
    // (no upper bound here: a batch's descriptors live in device memory; chv_composite splits a tick into launches of
    // at most CHV_MAX_LAYERS layers, the capacity of a slot of its descriptor ring)
    if (t.n_layers < 0 || t.n_layers > 4096) return fail(CHV_ERR_INVALID_VALUE, "%d layers", t.n_layers);
    if (t.n_layers > 0 && !t.layers) return fail(CHV_ERR_BAD_INPUT, "null layers");
    int tf = forced_target_format;
    int first = (int)layers->size();
    if (layers->capacity() < layers->size() + (size_t)t.n_layers) layers->reserve(std::max(layers->capacity() * 2, layers->size() + (size_t)t.n_layers));
    for (int i = 0; i < t.n_layers; i++) {
        DLayer dl;
        int rc = layer_to_device(t.layers[i], device, &tf, &dl);
        if (rc) return rc;
        layers->push_back(dl);
    }
    if (tf < 0) {
        // no layers: infer the clear flavour from the target's plane structure
        if (t.target.n_planes == 1) tf = TF_BGRA;
        else if (t.target.n_planes == 2) tf = TF_NV12;
        else if (t.target.n_planes == 3) tf = TF_Y420P;
        else return fail(CHV_ERR_BAD_TARGET, "target has %d planes", t.target.n_planes);
    }
    memset(dt, 0, sizeof *dt);
    int rc = target_to_device(&t.target, tf, device, &dt->dst);
    if (rc) return rc;
    dt->W = dt->dst.pl[0].w;
    dt->H = dt->dst.pl[0].h;
    // (the boxes are functions of the matrices, the kind, the flags and the canvas: a group of mixers repeats a handful of geometries a thousand
    // times per batch, a lone mixer the same ones every tick — the last few answers are kept per thread; a dozen double divisions per miss)
    struct BoxMemo { float m[48]; int32_t kind, flags, W, H, tf, bbox[4], ibox[4], flags_out; bool used; };
    static thread_local BoxMemo memo[8];
    static thread_local unsigned memo_next = 0;
    for (int i = first; i < (int)layers->size(); i++) {
        DLayer &L = (*layers)[i];
        BoxMemo *hit = nullptr;
        for (BoxMemo &M : memo)
            if (M.used && M.kind == L.kind && M.flags == L.flags && M.W == dt->W && M.H == dt->H && M.tf == tf && memcmp(M.m, L.u, sizeof M.m) == 0) { hit = &M; break; }
        if (hit) {
            memcpy(L.bbox, hit->bbox, sizeof L.bbox); memcpy(L.ibox, hit->ibox, sizeof L.ibox); L.flags = hit->flags_out;
        } else {
            BoxMemo &M = memo[memo_next++ & 7];
            memcpy(M.m, L.u, sizeof M.m); M.kind = L.kind; M.flags = L.flags; M.W = dt->W; M.H = dt->H; M.tf = tf;
            if (L.kind == LK_BGRA_METAL) { L.bbox[0] = 0; L.bbox[1] = 0; L.bbox[2] = dt->W; L.bbox[3] = dt->H; }
            else layer_bbox(&L, dt->W, dt->H);
            layer_inner_box(&L, dt->W, dt->H, tf);
            memcpy(M.bbox, L.bbox, sizeof L.bbox); memcpy(M.ibox, L.ibox, sizeof L.ibox); M.flags_out = L.flags; M.used = true;
        }
        if ((L.flags & LF_COVERS) && i - first < 31) dt->cover_mask |= 1 << (i - first);
    }
    // LF_SAME_GEOM (device_types.h): a layer whose geometry inputs equal its predecessor's
    if (switches().same_geom.load(std::memory_order_relaxed)) {
        for (int i = first + 1; i < (int)layers->size(); i++) {
            DLayer &L = (*layers)[i];
            const DLayer &P = (*layers)[i - 1];
            bool same = L.kind == P.kind && L.kind != LK_BGRA_METAL && memcmp(L.u, P.u, 48 * sizeof(float)) == 0 &&
                        memcmp(L.bbox, P.bbox, sizeof L.bbox) == 0 &&
                        ((L.flags ^ P.flags) & (LF_AXIS_ALIGNED | LF_BOUNDED)) == 0;
            for (int p = 0; p < 3 && same; p++) {
                const DPlane &a = L.src.pl[p], &b = P.src.pl[p];
                same = a.w == b.w && a.h == b.h && a.pitch == b.pitch && a.comps == b.comps && (a.ptr == nullptr) == (b.ptr == nullptr);
            }
            if (same) L.flags |= LF_SAME_GEOM;
        }
    }
    dt->clear_first = t.clear_first ? 1 : 0;
    dt->n_layers = t.n_layers;
    dt->first_layer = first;
    *target_format_out = tf;
    return CHV_OK;
}

// One slot of the descriptor ring for the lifetime of the object: taken once the device is done with what the slot's group held (see
// DescGroup), given back on EVERY path out of the scope — a launch that fails after taking the group's last slot still leaves the event
// (or the `unguarded` mark) behind the launches of the group that were queued before it.  The walk advances only when the wait succeeded.
struct DescSlot {
    chv_context *c;
    int slot = -1;
    int rc = CHV_OK;
    explicit DescSlot(chv_context *ctx) : c(ctx) {
        const int s = c->next_desc;
        DescGroup &g = c->desc_group[s / kDescGroup];
        if (s % kDescGroup == 0) {
            hipError_t e = hipSuccess;
            if (g.unguarded) e = hipStreamSynchronize(c->stream);
            else if (g.pending) e = hipEventSynchronize(g.done);
            if (e != hipSuccess) { rc = hip_fail(e, "waiting for a descriptor slot"); return; }
            g.pending = false; g.unguarded = false;
        }
        c->next_desc = (s + 1) % kDescSlots;
        slot = s;
    }
    ~DescSlot() {
        if (slot < 0 || slot % kDescGroup != kDescGroup - 1) return;
        DescGroup &g = c->desc_group[slot / kDescGroup];
        hipError_t e = hipSuccess;
        if (!g.done) e = hipEventCreateWithFlags(&g.done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(g.done, c->stream);
        if (e == hipSuccess) g.pending = true;
        else { g.pending = false; g.unguarded = true; (void)hipGetLastError(); }
    }
    DescSlot(const DescSlot &) = delete;
    DescSlot &operator=(const DescSlot &) = delete;
};

// launch one transient tick through the pinned descriptor ring
static int launch_transient(chv_context *c, const DTick &tick_in, const std::vector<DLayer> &layers, int tf) {
    HIP_TRY(hipSetDevice(c->device));
    // the tick as the kernels see it: first_layer = 0, its layers behind it
    DTick tick = tick_in;
    tick.first_layer = 0;
    const DTick *ht = &tick;
    const DLayer *hl = layers.data();
    // Where the kernel reads the descriptors from.  Every wave of the launch fetches its tick and, layer by layer, that layer's
    // planes, uniforms and flags with scalar loads — a handful of dependent loads per layer.  From the pinned host ring each of them
    // is a trip across PCIe (~1.5 us, uncached): a 4-layer 720p tick took 31 us of kernel time, 5 us per layer, whatever was done on
    // the chip (tools/tick_latency.py).  So the slot is copied to its twin in device memory on the launch's own stream first
    // (one small asynchronous copy), and the waves read L2 / scalar-cache resident descriptors.  CHV_DESC=host keeps the old way (A/B).
    // The streaming kernel goes one better for a lone tick: its descriptors travel as kernel ARGUMENTS (tick_bgra_stream_one) — no copy
    // in front of the launch, and every field a scalar load from one base instead of the tick -> layer chain.  CHV_DESC=device keeps the
    // copy for it too (A/B).
    const size_t used = sizeof(DTick) + layers.size() * sizeof(DLayer);
    const int desc_mode = switches().desc_host.load(std::memory_order_relaxed);       // 0 default, 1 host ring, 2 device twin always
    int path = select_fast_path(tf, ht, hl, 1, desc_mode == 0);
    (void)hipGetLastError();   // the launchers report through hipGetLastError(): drop whatever an earlier, unrelated call left there
    if (fast_path_by_value(path) && desc_mode == 0) {
        // descriptors as kernel arguments: the ring is not involved
        hipError_t e = launch_tick_fast(path, ht, hl, nullptr, nullptr, 1, ht->W, ht->H, c->stream, nullptr);
        return e == hipSuccess ? CHV_OK : hip_fail(e, "kernel launch");
    }
    // The strip kernels take a lone tick of up to WAVE_ONE_LAYERS layers as an ARGUMENT (wave_common.hip.h: wave_one_descriptors; tick_bgra_wave_one): no ring
    // slot, no copy in front of the launch.  The layers are pointed at the device's geometry tables first, where its store has them for this
    // scene; a launch that is to BUILD tables (a scene's second sighting) needs its layers in device memory and goes through the slot below.
    const bool wave = fast_path_is_wave(path);
    // what the store answered: built + patched where it pointed the layers at its tables for `config` (owns nothing, has no layer arrays)
    GeomCache covered;
    covered.owns = false; covered.n_layers = (int)layers.size();
    if (wave && desc_mode == 0 && wave_layers_by_value(tf, &tick, layers.data())) {
        WaveOne one;
        one.t = tick;
        memcpy(one.l, layers.data(), layers.size() * sizeof(DLayer));
        bool build = false;
        covered.built = covered.patched = geom_store_patch(tf, &one.t, one.l, 1, one.t.W, one.t.H, covered.n_layers, &covered.config, &build);
        if (!build) {
            hipError_t e = launch_tick_fast(path, &one.t, one.l, nullptr, nullptr, 1, one.t.W, one.t.H, c->stream, &covered);
            return e == hipSuccess ? CHV_OK : hip_fail(e, "kernel launch");
        }
    }
    DescSlot ds(c);
    if (ds.rc) return ds.rc;
    const int slot = ds.slot;
    uint8_t *base = c->desc_host + (size_t)slot * kDescSlotBytes;
    DTick *st = (DTick *)base;
    DLayer *sl = (DLayer *)(base + sizeof(DTick));
    *st = tick;
    if (!layers.empty()) memcpy(sl, layers.data(), layers.size() * sizeof(DLayer));
    // the strip kernels' geometry tables, where the device's store has them for this scene: the layers are pointed at them before they travel
    // (not with CHV_DESC=host: a build would copy the slot onto itself)
    bool build_tables = false;
    if (wave && !layers.empty() && desc_mode != 1)
        covered.built = covered.patched = geom_store_patch(tf, st, sl, 1, st->W, st->H, covered.n_layers, &covered.config, &build_tables);
    DTick *dt = nullptr;
    if (desc_mode == 1) {
        HIP_TRY(hipHostGetDevicePointer((void **)&dt, st, 0));
    } else {
        dt = (DTick *)(c->desc_dev + (size_t)slot * kDescSlotBytes);
        HIP_TRY(hipMemcpyAsync(dt, st, used, hipMemcpyHostToDevice, c->stream));
    }
    DLayer *dl = (DLayer *)((uint8_t *)dt + sizeof(DTick));
    hipError_t e;
    if (build_tables) {
        // a geometry the device's store has been asked for before and does not have yet: this launch builds its tables (as a batch's second launch
        // does) and gives them to the store — the next tick of the scene finds them before its descriptors are copied
        GeomCache tmp;
        tmp.d_layers = dl; tmp.h_layers = sl; tmp.n_layers = (int)layers.size(); tmp.force_build = true;
        e = launch_tick_fast(path, st, sl, dt, dl, 1, st->W, st->H, c->stream, &tmp);
        if (tmp.owns && tmp.tables) (void)hipStreamSynchronize(c->stream);          // (the store was full: the tables die with this launch)
        geom_cache_release(tmp);
    } else {
        e = path >= 0 ? launch_tick_fast(path, st, sl, dt, dl, 1, st->W, st->H, c->stream, &covered)
                      : launch_tick_general(tf, st, sl, dt, dl, 1, st->W, st->H, c->stream);
    }
    if (e != hipSuccess) return hip_fail(e, "kernel launch");
    return CHV_OK;
}

// ---------------------------------------------------------------------------
// passes and kernels
// ---------------------------------------------------------------------------
static int composite_now(chv_context *c, const chv_image *target, int clear_first, int forced_tf, const chv_layer *layers, int n_layers);

static void pending_release(chv_context *c) {
    std::vector<chv_buffer *> dead;
    {
        std::lock_guard<std::mutex> lock(g_pin_mu);
        for (chv_buffer *b : c->pending.pins)
            if (--b->pins == 0 && b->doomed) dead.push_back(b);
    }
    for (chv_buffer *b : dead) (void)buffer_free_now(b);          // (hipFree waits for the launch that just went out)
    c->pending.pins.clear();
    c->pending.layers.clear();
    c->pending.active = false;
    c->pending.clear_first = 0;
    c->pending.clear_tf = -1;
}

// Launch what the pass has accepted so far.  Called by every entry point that puts work on the context's stream, hands the stream out, or
// waits for it — the pending kernels keep their place in the stream's order.  Their arguments were validated when they were accepted, so what
// can still fail here is the launch itself.
static int flush_pending(chv_context *c) {
    if (!c->pending.active) return CHV_OK;
    const int rc = composite_now(c, &c->pending.target, c->pending.clear_first, c->pending.clear_tf,
                                 c->pending.layers.empty() ? nullptr : c->pending.layers.data(), (int)c->pending.layers.size());
    pending_release(c);
    return rc;
}

static bool same_target(const chv_image &a, const chv_image &b) {
    if (a.n_planes != b.n_planes) return false;
    for (int i = 0; i < a.n_planes && i < 3; i++) {
        const chv_plane &p = a.planes[i], &q = b.planes[i];
        if (p.buffer != q.buffer || p.offset != q.offset || p.pitch != q.pitch || p.width != q.width || p.height != q.height || p.components != q.components)
            return false;
    }
    return true;
}

extern "C" int chv_pass_begin(chv_context *c) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    // no device work: like OpenCL, a pass is just a bracket (compute.cl.swift:234-237).  Brackets nest (uploadComputePicture opens its own,
    // compute.cl.swift:433,453, downloadComputePicture :470,492): kernels are held while any is open, every chv_pass_end launches what is held
    if (c->pass_depth < (1 << 20)) c->pass_depth++;
    return CHV_OK;
}

extern "C" int chv_pass_end(chv_context *c, int wait) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (c->pass_depth > 0) c->pass_depth--;
    HIP_TRY(hipSetDevice(c->device));
    // the pass's picture kernels, held back since chv_run_kernel accepted them: one fused launch where they are `clear + layers on one target`
    FLUSH_PENDING(c);
    // (hipStreamSynchronize already polls before it blocks: a hand-written hipStreamQuery loop in front of it measured the
    // same 16-17 us for an empty tick, tools/tick_latency.py — that floor is the launch + completion path of the runtime)
    if (wait) HIP_TRY(hipStreamSynchronize(c->stream));
    else (void)hipStreamQuery(c->stream);  // nudge submission, the clFlush analogue
    return CHV_OK;
}

// snd_s16i_s16i / me_fullsearch (kernels_idle.hip.cpp): buffers and luma planes bound as the reference binds them, no tick descriptors
static int run_idle_kernel(chv_context *c, int kernel, const chv_image *target, const chv_image *inputs, int n_inputs,
                           const void *uniforms, size_t uniforms_size) {
    FLUSH_PENDING(c);
    DepScope deps;
    if (target->n_planes < 1) return fail(CHV_ERR_BAD_TARGET, "%s: target without planes", chv_kernel_name(kernel));
    if (n_inputs < 0 || (n_inputs > 0 && !inputs)) return fail(CHV_ERR_BAD_INPUT, "null inputs");
    for (int i = 0; i < n_inputs; i++) if (inputs[i].n_planes < 1) return fail(CHV_ERR_BAD_INPUT, "%s: input %d has no planes", chv_kernel_name(kernel), i);
    int rc;
    if (kernel == CHV_K_SND_S16I_S16I) {
        if (!uniforms || uniforms_size != sizeof(chv_snd_uniforms))
            return fail(CHV_ERR_INVALID_VALUE, "snd_s16i_s16i needs the 100-byte BufferUniforms, got %zu bytes", uniforms_size);
        chv_snd_uniforms u;
        memcpy(&u, uniforms, sizeof u);
        if (u.input_count < 0 || u.input_count > 8) return fail(CHV_ERR_INVALID_VALUE, "snd_s16i_s16i: inputCount %d", u.input_count);
        if (n_inputs < u.input_count) return fail(CHV_ERR_BAD_INPUT, "snd_s16i_s16i: inputCount %d, %d buffers given", u.input_count, n_inputs);
        DPlane out;
        if ((rc = plane_to_device(target->planes[0], 2, c->device, &out, CHV_ERR_BAD_TARGET, "target", 0))) return rc;
        if (out.h > 1 && out.pitch != out.w * 2) return fail(CHV_ERR_BAD_TARGET, "snd_s16i_s16i: rows of samples must be contiguous");
        if (((uintptr_t)out.ptr) & 1) return fail(CHV_ERR_BAD_TARGET, "snd_s16i_s16i: samples must be 2-byte aligned");
        // the kernel's sample count is an int (the reference's get_global_size(0)): a buffer of 2^31 samples or more is refused, not truncated
        if ((int64_t)out.w * (int64_t)out.h > (int64_t)INT32_MAX)
            return fail(CHV_ERR_BAD_TARGET, "snd_s16i_s16i: %lld samples exceed the kernel's 32-bit count", (long long)((int64_t)out.w * out.h));
        const size_t span = (size_t)out.w * (size_t)out.h * 2;
        const int16_t *in[8] = { nullptr };
        for (int i = 0; i < u.input_count; i++) {
            DPlane p;
            if ((rc = plane_to_device(inputs[i].planes[0], 2, c->device, &p, CHV_ERR_BAD_INPUT, "input", i))) return rc;
            if (p.w != out.w || p.h != out.h || (p.h > 1 && p.pitch != p.w * 2) || (((uintptr_t)p.ptr) & 1))
                return fail(CHV_ERR_BAD_INPUT, "snd_s16i_s16i: input %d does not have the output's shape", i);
            // The source accumulates INTO out[gid] input after input (kernels.cl.swift:548-560), so an input that is the output would read the
            // partially mixed sample; the kernel keeps the accumulator in a register and reads every input once.  Not a case any caller has
            // (the inputs are other tracks' buffers): overlapping buffers are refused rather than mixed differently.
            if ((uintptr_t)p.ptr < (uintptr_t)out.ptr + span && (uintptr_t)out.ptr < (uintptr_t)p.ptr + span)
                return fail(CHV_ERR_BAD_INPUT, "snd_s16i_s16i: input %d overlaps the output buffer", i);
            in[i] = (const int16_t *)p.ptr;
        }
        auto dp = deps.deps();
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = wait_for_uploads(c->stream, dp))) return rc;
        HIP_TRY(launch_snd_s16i((int16_t *)out.ptr, in, u.input_count, out.w * out.h, u.input_gains, u.input_fade, c->stream));
        return CHV_OK;
    }
    if (!uniforms || uniforms_size != sizeof(chv_me_uniforms))
        return fail(CHV_ERR_INVALID_VALUE, "me_fullsearch needs the 24-byte MotionEstimationUniforms, got %zu bytes", uniforms_size);
    chv_me_uniforms u;
    memcpy(&u, uniforms, sizeof u);
    if (n_inputs != 2) return fail(CHV_ERR_BAD_INPUT, "me_fullsearch takes the reference and the current picture, got %d images", n_inputs);
    if (u.block_size[0] < 1 || u.block_size[1] < 1 || u.block_size[0] > 64 || u.block_size[1] > 64 || u.search_window_size[0] < 0 || u.search_window_size[1] < 0)
        return fail(CHV_ERR_INVALID_VALUE, "me_fullsearch: block %dx%d, window %dx%d", u.block_size[0], u.block_size[1], u.search_window_size[0], u.search_window_size[1]);
    DPlane out, ref, cur;
    if ((rc = plane_to_device(target->planes[0], 4, c->device, &out, CHV_ERR_BAD_TARGET, "target", 0))) return rc;
    if ((rc = plane_to_device(inputs[0].planes[0], 1, c->device, &ref, CHV_ERR_BAD_INPUT, "reference picture", 0))) return rc;
    if ((rc = plane_to_device(inputs[1].planes[0], 1, c->device, &cur, CHV_ERR_BAD_INPUT, "current picture", 0))) return rc;
    // deltaCost2 (kernels.metal:135-142) per vector component, by |v|: lambda * (log2(|v| + 1) * 2 + 0.718 + (v != 0)) + 0.5 through the HOST's
    // log2f, the table oracle/ref_kernels.c builds the same way — no device libm in the comparison
    static float cost[256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int d = 0; d < 256; d++) {
            const float l2 = log2f((float)d + 1.0f), rounding = d != 0 ? 1.0f : 0.0f;
            cost[d] = 4.0f * (l2 * 2.0f + 0.718f + rounding) + 0.5f;
        }
    });
    auto dp = deps.deps();
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = wait_for_uploads(c->stream, dp))) return rc;
    HIP_TRY(launch_me_fullsearch(out, ref, cur, u.block_size, u.search_window_size, u.image_size, cost, c->stream));
    return CHV_OK;
}

extern "C" int chv_run_kernel(chv_context *c, int kernel, const chv_image *target,
                              const chv_image *inputs, int n_inputs,
                              const void *uniforms, size_t uniforms_size, int blends,
                              const chv_kernel_opts *opts) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (!target) return fail(CHV_ERR_BAD_TARGET, "null target");
    if (kernel == CHV_K_SND_S16I_S16I || kernel == CHV_K_ME_FULLSEARCH) return run_idle_kernel(c, kernel, target, inputs, n_inputs, uniforms, uniforms_size);
    KernelShape s;
    int rc = kernel_shape(kernel, &s);
    if (rc) return rc;
    chv_tick t;
    memset(&t, 0, sizeof t);
    t.target = *target;
    chv_layer layer;
    if (s.is_clear) {
        t.clear_first = 1;
        t.n_layers = 0;
    } else {
        if (n_inputs != 1 || !inputs)
            return fail(CHV_ERR_BAD_INPUT, "%s takes exactly one input image, got %d", chv_kernel_name(kernel), n_inputs);
        if (!uniforms || uniforms_size != sizeof(chv_uniforms))
            return fail(CHV_ERR_INVALID_VALUE, "%s needs the 236-byte ImageUniforms, got %zu bytes", chv_kernel_name(kernel), uniforms_size);
        if (!blends)
            return fail(CHV_ERR_INVALID_OPERATION, "%s reads the current target; call it with blends = true", chv_kernel_name(kernel));
        memset(&layer, 0, sizeof layer);
        layer.kernel = kernel;
        layer.image = inputs[0];
        memcpy(&layer.uniforms, uniforms, sizeof(chv_uniforms));
        if (opts) layer.opts = *opts;
        t.clear_first = 0;
        t.n_layers = 1;
        t.layers = &layer;
    }
    DTick dt;
    std::vector<DLayer> dl;
    int tf = -1;
    DepScope deps;
    rc = tick_to_device(t, c->device, s.is_clear ? s.target_format : -1, &dt, &dl, &tf);      // (every argument error surfaces here, in this call)
    if (rc) return rc;
    if (c->pass_depth > 0 && switches().pass_fuse.load(std::memory_order_relaxed)) {
        // Inside a pass: accept the kernel, launch it with the rest of the pass (flush_pending).  A kernel on another target, or a clear
        // after something else, first sends out what is held — the stream sees the kernels in the order they were issued.
        chv_context::PendingPass &pp = c->pending;
        // ... and so does a layer that READS the canvas being held (issued kernel by kernel it would sample what the held layers wrote; inside one
        // fused launch the canvas lives in registers and memory still has the old bytes), and a pass deeper than a batch's descriptor allows
        // (by device ADDRESS RANGE, not by handle: a second chv_buffer_wrap over the canvas's memory, or a view with plane offsets, reads it too)
        bool reads_held_canvas = false;
        if (pp.active && !s.is_clear)
            for (int n = 0; n < n_inputs; n++)
                for (int i = 0; i < inputs[n].n_planes && i < 3; i++)
                    for (int k = 0; k < pp.target.n_planes && k < 3; k++)
                        reads_held_canvas = reads_held_canvas || planes_overlap(inputs[n].planes[i], pp.target.planes[k]);
        if (pp.active && (s.is_clear || reads_held_canvas || pp.layers.size() >= 1024 || !same_target(pp.target, *target) || (pp.clear_tf >= 0 && pp.clear_tf != tf)))
            FLUSH_PENDING(c);
        if (!pp.active) {
            pp.active = true;
            pp.target = *target;
            pp.clear_first = 0;
            pp.clear_tf = -1;
        }
        if (s.is_clear) { pp.clear_first = 1; pp.clear_tf = s.target_format; }
        else pp.layers.push_back(layer);
        {
            std::lock_guard<std::mutex> lock(g_pin_mu);
            for (chv_buffer *b : deps.bufs) { b->pins++; pp.pins.push_back(b); }
        }
        return CHV_OK;
    }
    FLUSH_PENDING(c);
    auto dp = deps.deps();
    rc = wait_for_uploads(c->stream, dp);
    if (rc) return rc;
    return launch_transient(c, dt, dl, tf);
}

extern "C" int chv_composite(chv_context *c, const chv_image *target, int clear_first,
                             const chv_layer *layers, int n_layers) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (!target) return fail(CHV_ERR_BAD_TARGET, "null target");
    if (n_layers < 0) return fail(CHV_ERR_INVALID_VALUE, "%d layers", n_layers);
    if (n_layers > 0 && !layers) return fail(CHV_ERR_BAD_INPUT, "null layers");
    FLUSH_PENDING(c);
    return composite_now(c, target, clear_first, -1, layers, n_layers);
}

// (`forced_tf`: the target format a clear kernel of a deferred pass fixed; -1: the layers' kernels decide, the plane count if there are none)
static int composite_now(chv_context *c, const chv_image *target, int clear_first, int forced_tf, const chv_layer *layers, int n_layers) {
    // A mixer composes any number of layers (mix.video.swift:116-124).  One launch takes up to CHV_MAX_LAYERS of them;
    // a deeper tick becomes several launches on the context's stream — the first clears, the others continue on the
    // canvas.  Byte-identical to one pass: the canvas is re-quantised between layers either way.
    // All chunks are validated before the first one is launched, so a bad layer leaves the canvas untouched.
    const int n_chunks = n_layers <= CHV_MAX_LAYERS ? 1 : (n_layers + CHV_MAX_LAYERS - 1) / CHV_MAX_LAYERS;
    std::vector<DTick> dts((size_t)n_chunks);
    std::vector<std::vector<DLayer>> dls((size_t)n_chunks);
    int tf = forced_tf;
    DepScope deps;
    for (int k = 0; k < n_chunks; k++) {
        chv_tick t;
        memset(&t, 0, sizeof t);
        t.target = *target;
        t.clear_first = k == 0 ? clear_first : 0;
        t.n_layers = std::min(CHV_MAX_LAYERS, n_layers - k * CHV_MAX_LAYERS);
        t.layers = layers ? layers + (size_t)k * CHV_MAX_LAYERS : nullptr;
        int tfk = tf;
        int rc = tick_to_device(t, c->device, tf, &dts[k], &dls[k], &tfk);
        if (rc) return rc;
        tf = tfk;
    }
    auto dp = deps.deps();
    int rc = wait_for_uploads(c->stream, dp);
    if (rc) return rc;
    for (int k = 0; k < n_chunks; k++) {
        rc = launch_transient(c, dts[k], dls[k], tf);
        if (rc) return rc;
    }
    return CHV_OK;
}

// ---------------------------------------------------------------------------
// batches
// ---------------------------------------------------------------------------
extern "C" int chv_batch_create(chv_context *c, const chv_tick *ticks, int n_ticks, chv_batch **out) {
    if (!out) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    *out = nullptr;
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (!ticks || n_ticks <= 0) return fail(CHV_ERR_INVALID_VALUE, "empty batch");
    if (n_ticks > 65535) return fail(CHV_ERR_INVALID_VALUE, "at most 65535 ticks per batch");
    std::vector<DTick> dts((size_t)n_ticks);
    std::vector<DLayer> dls;
    {
        size_t total = 0;
        for (int i = 0; i < n_ticks; i++) total += ticks[i].n_layers > 0 && ticks[i].n_layers <= 4096 ? (size_t)ticks[i].n_layers : 0;
        dls.reserve(total);
    }
    int tf0 = -1, maxW = 0, maxH = 0;
    DepScope deps;
    deps.bufs.reserve((size_t)n_ticks * 3 + dls.capacity() * 3);
    for (int i = 0; i < n_ticks; i++) {
        int tf = -1;
        int rc = tick_to_device(ticks[i], c->device, -1, &dts[i], &dls, &tf);
        if (rc) return rc;
        if (tf0 < 0) tf0 = tf;
        else if (tf != tf0) return fail(CHV_ERR_BAD_TARGET, "all ticks of a batch must share the target format");
        if (dts[i].W > maxW) maxW = dts[i].W;
        if (dts[i].H > maxH) maxH = dts[i].H;
    }
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<chv_batch> b(new chv_batch);
    b->device = c->device; b->n_ticks = n_ticks; b->n_layers = (int)dls.size();
    b->target_format = tf0; b->maxW = maxW; b->maxH = maxH;
    // Everything that decides what the descriptors look like happens on the host first — the route, a split into two launches, the geometry
    // tables the device's store has for the scene — so that they travel once.
    b->fast_path = select_fast_path(tf0, dts.data(), dls.data(), n_ticks);
    auto path_name = [&](int path) { return path >= 0 ? std::string(fast_path_name(path))
                                                       : std::string(tf0 == TF_BGRA ? "tick_general_bgra" : (tf0 == TF_NV12 ? "tick_general_yuv<nv12>" : "tick_general_yuv<y420p>")); };
    b->kernel_name = path_name(b->fast_path);
    if (tf0 == TF_BGRA && b->fast_path != fast_path_stream_bgra()) {
        const int k = split_stream_prefix(dts.data(), dls.data(), n_ticks);
        if (k > 0) {
            std::vector<DTick> head = dts, tail = dts;
            for (int i = 0; i < n_ticks; i++) {
                head[(size_t)i].n_layers = k;
                head[(size_t)i].cover_mask &= (1 << k) - 1;
                tail[(size_t)i].first_layer += k; tail[(size_t)i].n_layers -= k; tail[(size_t)i].clear_first = 0;
                tail[(size_t)i].cover_mask = (int32_t)((uint32_t)tail[(size_t)i].cover_mask >> k);
            }
            const int p1 = select_fast_path(tf0, head.data(), dls.data(), n_ticks), p2 = select_tail_path(tf0, tail.data(), dls.data(), n_ticks);
            if (p1 == fast_path_stream_bgra()) {
                b->fast_path = p1; b->fast_path2 = p2;
                b->h_ticks2 = std::move(tail);
                dts = std::move(head);
                b->kernel_name = path_name(p1) + " + " + path_name(p2);
            }
        }
    }
    // The strip kernels' geometry tables, where the device's store has them for this scene (a batch is bound to its pictures: a host builds one per
    // group of frames, and the second one of a scene onwards starts with tables): the layers are pointed at them before they are sent.
    {
        const bool w1 = fast_path_is_wave(b->fast_path), w2 = b->fast_path2 != -2 && fast_path_is_wave(b->fast_path2);
        if ((w1 || w2) && !dls.empty()) {
            GeomConfig cfg{};
            bool want_build = false;
            const std::vector<DTick> &tk = w1 ? dts : b->h_ticks2;
            if (geom_store_patch(tf0, tk.data(), dls.data(), n_ticks, b->maxW, b->maxH, (int)dls.size(), &cfg, &want_build)) {
                b->geom.built = true; b->geom.patched = true; b->geom.config = cfg; b->geom.owns = false; b->geom.tables = nullptr;
            }
        }
    }
    // ticks | layers | the second launch's ticks: one block of the device's pool (DescBlock), one asynchronous copy on this context's stream
    const size_t tb = sizeof(DTick) * dts.size(), lb = sizeof(DLayer) * (dls.size() ? dls.size() : 1), t2b = sizeof(DTick) * b->h_ticks2.size();
    const size_t lo = (tb + 255) & ~(size_t)255, t2o = (lo + lb + 255) & ~(size_t)255, total = t2o + t2b;
    hipError_t e = hipSuccess;
    if (desc_block_acquire(c->device, total, &b->blk)) {
        DescBlock &K = b->blk;
        if (K.recorded) e = hipEventSynchronize(K.ev);                 // (its last user's copy and launches: long done for a host that waited for its tick)
        if (e == hipSuccess) {
            memcpy(K.host, dts.data(), tb);
            if (!dls.empty()) memcpy(K.host + lo, dls.data(), sizeof(DLayer) * dls.size());
            if (t2b) memcpy(K.host + t2o, b->h_ticks2.data(), t2b);
            e = hipMemcpyAsync(K.dev, K.host, total, hipMemcpyHostToDevice, c->stream);
        }
        if (e == hipSuccess) e = hipEventRecord(K.ev, c->stream);
        if (e != hipSuccess) { desc_block_release(c->device, K); return hip_fail(e, "descriptors of a batch"); }
        K.recorded = true; K.last = c->stream;
        b->d_ticks = (DTick *)K.dev; b->d_layers = (DLayer *)(K.dev + lo); b->d_ticks2 = t2b ? (DTick *)(K.dev + t2o) : nullptr;
        b->lo = lo; b->t2o = t2o; b->used = total;
    } else {
        e = hipMalloc((void **)&b->d_ticks, tb);
        if (e == hipSuccess) e = hipMalloc((void **)&b->d_layers, lb);
        if (e == hipSuccess && t2b) e = hipMalloc((void **)&b->d_ticks2, t2b);
        if (e == hipSuccess) e = hipMemcpy(b->d_ticks, dts.data(), tb, hipMemcpyHostToDevice);
        if (e == hipSuccess && !dls.empty()) e = hipMemcpy(b->d_layers, dls.data(), sizeof(DLayer) * dls.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && t2b) e = hipMemcpy(b->d_ticks2, b->h_ticks2.data(), t2b, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (b->d_ticks) (void)hipFree(b->d_ticks);
            if (b->d_layers) (void)hipFree(b->d_layers);
            if (b->d_ticks2) (void)hipFree(b->d_ticks2);
            return hip_fail(e, "descriptors of a batch");
        }
    }
    b->h_ticks = std::move(dts);
    b->h_layers = std::move(dls);
    b->deps = deps.deps();
    // what chv_batch_rebind compares a replacement with, and the buffer behind every plane (`deps` is recomputed from these after a rebind)
    {
        const size_t n_slots = (size_t)n_ticks + b->h_layers.size();
        b->slot_meta.resize(n_slots);
        b->slot_bufs.assign(n_slots * 3, nullptr);
        b->slot_stamp.assign(n_slots, 0);
        for (int i = 0; i < n_ticks; i++) {
            const chv_image &T = ticks[i].target;
            b->slot_meta[(size_t)i] = chv_batch::SlotMeta{ T.format, T.width, T.height, T.n_planes };
            for (int p = 0; p < 3; p++) if (b->h_ticks[(size_t)i].dst.pl[p].ptr) b->slot_bufs[(size_t)i * 3 + p] = T.planes[p].buffer;
            const size_t first = (size_t)b->h_ticks[(size_t)i].first_layer;
            for (int l = 0; l < ticks[i].n_layers; l++) {
                const chv_image &I = ticks[i].layers[l].image;
                const size_t s = (size_t)n_ticks + first + (size_t)l;
                b->slot_meta[s] = chv_batch::SlotMeta{ I.format, I.width, I.height, I.n_planes };
                for (int p = 0; p < 3; p++) if (b->h_layers[first + (size_t)l].src.pl[p].ptr) b->slot_bufs[s * 3 + p] = I.planes[p].buffer;
            }
        }
    }
    *out = b.release();
    return CHV_OK;
}

extern "C" int chv_batch_run(chv_context *c, chv_batch *b) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (!b || !b->d_ticks) return fail(CHV_ERR_INVALID_VALUE, "bad batch");
    if (b->device != c->device) return fail(CHV_ERR_INVALID_CONTEXT, "batch belongs to device %d", b->device);
    HIP_TRY(hipSetDevice(c->device));
    int wrc = wait_for_uploads(c->stream, b->deps);
    if (wrc) return wrc;
    (void)hipGetLastError();   // see launch_transient
    // (pooled descriptors: their copy went out on the creating context's stream, and the block's event marks the last thing that used it)
    if (b->blk.dev && b->blk.last != c->stream) HIP_TRY(hipStreamWaitEvent(c->stream, b->blk.ev, 0));
    // ... and on every way out from here the block's event goes behind whatever this call queued (the launchers may queue more than the tick
    // kernels — a table build —, and a failing second launch leaves the first one in flight): what the next user of the block waits for
    struct BlockMark {
        chv_batch *bb; hipStream_t st;
        ~BlockMark() { if (bb->blk.dev) { if (hipEventRecord(bb->blk.ev, st) == hipSuccess) bb->blk.last = st; else (void)hipGetLastError(); } }
    } mark{ b, c->stream };
    // (the layer arrays the strip kernels' launcher patches when it builds the batch's geometry tables: geom_cache.h)
    b->geom.d_layers = b->d_layers; b->geom.h_layers = b->h_layers.data(); b->geom.n_layers = (int)b->h_layers.size();
    hipError_t e = b->fast_path >= 0
        ? launch_tick_fast(b->fast_path, b->h_ticks.data(), b->h_layers.data(), b->d_ticks, b->d_layers, b->n_ticks, b->maxW, b->maxH, c->stream, &b->geom)
        : launch_tick_general(b->target_format, b->h_ticks.data(), b->h_layers.data(), b->d_ticks, b->d_layers, b->n_ticks, b->maxW, b->maxH, c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch");
    if (b->fast_path2 != -2) {
        e = b->fast_path2 >= 0
            ? launch_tick_fast(b->fast_path2, b->h_ticks2.data(), b->h_layers.data(), b->d_ticks2, b->d_layers, b->n_ticks, b->maxW, b->maxH, c->stream, &b->geom)
            : launch_tick_general(b->target_format, b->h_ticks2.data(), b->h_layers.data(), b->d_ticks2, b->d_layers, b->n_ticks, b->maxW, b->maxH, c->stream);
        if (e != hipSuccess) return hip_fail(e, "kernel launch (second part of the batch)");
    }
    return CHV_OK;
}

// Point slots of a batch at new pictures (chipvideo.h).  Nothing but DPlane::ptr fields changes: every item is checked against what its slot was
// created with (same format, plane sizes, pitches, components; same address residue modulo 16 on the fast routes, which were chosen under
// aligned16-style conditions), then the new addresses go to the device — by the scatter kernel (rebind.h) or as the whole block again —, ordered
// on c's stream behind every earlier run of the batch, and only then the host copies, the per-slot buffers and `deps` follow.
extern "C" int chv_batch_rebind(chv_context *c, chv_batch *b, const chv_rebind *items, int n_items) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (!b || !b->d_ticks) return fail(CHV_ERR_INVALID_VALUE, "bad batch");
    if (n_items < 0 || (n_items > 0 && !items)) return fail(CHV_ERR_INVALID_VALUE, "null items");
    if (b->device != c->device) return fail(CHV_ERR_INVALID_CONTEXT, "batch belongs to device %d", b->device);
    if (n_items == 0) return CHV_OK;
    const bool fast = b->fast_path >= 0 || b->fast_path2 >= 0;
    const bool split = !b->h_ticks2.empty();
    if (++b->rebind_gen == 0) { std::fill(b->slot_stamp.begin(), b->slot_stamp.end(), 0u); b->rebind_gen = 1; }
    struct NewPlane { uint32_t slot; int32_t p; uint8_t *ptr; chv_buffer *buf; };
    static thread_local std::vector<NewPlane> np;
    static thread_local std::vector<RebindItem> list;
    np.clear(); list.clear();
    const size_t tick_plane = offsetof(DTick, dst) + offsetof(DImage, pl), layer_plane = offsetof(DLayer, src) + offsetof(DImage, pl);
    // ---- every item is checked before anything changes
    for (int k = 0; k < n_items; k++) {
        const chv_rebind &it = items[k];
        if (it.tick < 0 || it.tick >= b->n_ticks) return fail(CHV_ERR_INVALID_VALUE, "item %d: tick %d of %d", k, it.tick, b->n_ticks);
        const DTick &T = b->h_ticks[(size_t)it.tick];
        const int n_layers = T.n_layers + (split ? b->h_ticks2[(size_t)it.tick].n_layers : 0);
        if (it.layer < -1 || it.layer >= n_layers) return fail(CHV_ERR_INVALID_VALUE, "item %d: layer %d of %d", k, it.layer, n_layers);
        const bool target = it.layer < 0;
        const size_t li = target ? 0 : (size_t)T.first_layer + (size_t)it.layer;
        const size_t slot = target ? (size_t)it.tick : (size_t)b->n_ticks + li;
        if (b->slot_stamp[slot] == b->rebind_gen) return fail(CHV_ERR_INVALID_VALUE, "item %d: tick %d, layer %d is named twice", k, it.tick, it.layer);
        b->slot_stamp[slot] = b->rebind_gen;
        const chv_batch::SlotMeta &M = b->slot_meta[slot];
        const chv_image &I = it.image;
        if (I.format != M.format || I.width != M.width || I.height != M.height || I.n_planes != M.n_planes)
            return fail(CHV_ERR_INVALID_VALUE, "item %d: a %dx%d picture of format %d with %d planes cannot take the place of a %dx%d one of format %d with %d: rebuild the batch",
                        k, I.width, I.height, I.format, I.n_planes, M.width, M.height, M.format, M.n_planes);
        const DImage &old = target ? T.dst : b->h_layers[li].src;
        for (int p = 0; p < 3; p++) {
            const DPlane &O = old.pl[p];
            if (!O.ptr) continue;
            DPlane N;
            int rc = plane_to_device(I.planes[p], O.comps, b->device, &N, target ? CHV_ERR_BAD_TARGET : CHV_ERR_BAD_INPUT, target ? "target" : "input", p);
            if (rc) return rc;
            if (N.w != O.w || N.h != O.h || N.pitch != O.pitch)
                return fail(CHV_ERR_INVALID_VALUE, "item %d, plane %d: %dx%d with pitch %d cannot take the place of %dx%d with pitch %d: rebuild the batch",
                            k, p, N.w, N.h, N.pitch, O.w, O.h, O.pitch);
            if (fast && ((((uintptr_t)N.ptr) ^ ((uintptr_t)O.ptr)) & 15))
                return fail(CHV_ERR_INVALID_VALUE, "item %d, plane %d: the batch's route (%s) was chosen for an address of another alignment: rebuild the batch",
                            k, p, b->kernel_name.c_str());
            np.push_back(NewPlane{ (uint32_t)slot, p, N.ptr, I.planes[p].buffer });
            const size_t in_image = (size_t)p * sizeof(DPlane) + offsetof(DPlane, ptr);
            if (target) {
                list.push_back(RebindItem{ (uint32_t)((size_t)it.tick * sizeof(DTick) + tick_plane + in_image), 0, (uint64_t)(uintptr_t)N.ptr });
                if (split) list.push_back(RebindItem{ (uint32_t)(b->t2o + (size_t)it.tick * sizeof(DTick) + tick_plane + in_image), 0, (uint64_t)(uintptr_t)N.ptr });
            } else {
                list.push_back(RebindItem{ (uint32_t)(b->lo + li * sizeof(DLayer) + layer_plane + in_image), 0, (uint64_t)(uintptr_t)N.ptr });
            }
        }
    }
    if (np.empty()) return CHV_OK;
    HIP_TRY(hipSetDevice(c->device));
    // the host copies with the new addresses (h_ticks / h_layers / h_ticks2 carry the table words the launcher patched: geom_cache.h)
    auto apply = [&](DTick *ht, DLayer *hl, DTick *ht2) {
        for (const NewPlane &n : np) {
            if (n.slot < (uint32_t)b->n_ticks) { ht[n.slot].dst.pl[n.p].ptr = n.ptr; if (ht2) ht2[n.slot].dst.pl[n.p].ptr = n.ptr; }
            else hl[n.slot - (uint32_t)b->n_ticks].src.pl[n.p].ptr = n.ptr;
        }
    };
    if (!b->blk.dev) {
        // allocations of its own (the pool was full when the batch was made): no event orders them against runs on other streams — the device is
        // drained, and the three arrays go again synchronously
        std::vector<DTick> nt = b->h_ticks, nt2 = b->h_ticks2;
        std::vector<DLayer> nl = b->h_layers;
        apply(nt.data(), nl.data(), split ? nt2.data() : nullptr);
        HIP_TRY(hipDeviceSynchronize());
        hipError_t e = hipMemcpy(b->d_ticks, nt.data(), sizeof(DTick) * nt.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !nl.empty()) e = hipMemcpy(b->d_layers, nl.data(), sizeof(DLayer) * nl.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && split) e = hipMemcpy(b->d_ticks2, nt2.data(), sizeof(DTick) * nt2.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            // put back what may have been overwritten: the batch runs as before the call
            (void)hipGetLastError();
            (void)hipMemcpy(b->d_ticks, b->h_ticks.data(), sizeof(DTick) * b->h_ticks.size(), hipMemcpyHostToDevice);
            if (!b->h_layers.empty()) (void)hipMemcpy(b->d_layers, b->h_layers.data(), sizeof(DLayer) * b->h_layers.size(), hipMemcpyHostToDevice);
            if (split) (void)hipMemcpy(b->d_ticks2, b->h_ticks2.data(), sizeof(DTick) * b->h_ticks2.size(), hipMemcpyHostToDevice);
            (void)hipGetLastError();
            return hip_fail(e, "descriptors of a batch (rebind)");
        }
    } else {
        DescBlock &K = b->blk;
        for (const RebindItem &r : list)
            if ((r.off & 7) || (size_t)r.off + 8 > b->used) return fail(CHV_ERR_UNKNOWN, "rebind: offset %u outside the block's %zu bytes", r.off, b->used);
        const RebindLauncher launcher = g_rebind_launcher.load(std::memory_order_acquire);
        const int mode = switches().rebind.load(std::memory_order_relaxed);
        const bool scatter = launcher && mode != 2;
        // before a pinned area is overwritten: the last stream operation that read it (a host that waited for its tick never blocks here)
        auto await_stage = [&](int i) -> hipError_t {
            if (!b->stage_ev[i]) return hipEventCreateWithFlags(&b->stage_ev[i], hipEventDisableTiming);
            if (!b->stage_pending[i]) return hipSuccess;
            hipError_t e = hipEventSynchronize(b->stage_ev[i]);
            if (e == hipSuccess) b->stage_pending[i] = false;
            return e;
        };
        int si = -1;
        hipError_t e = hipSuccess;
        const RebindItem *list_dev = nullptr;
        if (scatter && (int)list.size() > kRebindByValue) {
            si = b->next_stage;
            if ((e = await_stage(si)) != hipSuccess) return hip_fail(e, "rebind: waiting for the item list's last reader");
            if (b->stage_cap[si] < list.size()) {
                if (b->stage[si]) { (void)hipHostFree(b->stage[si]); b->stage[si] = nullptr; b->stage_dev[si] = nullptr; b->stage_cap[si] = 0; }
                size_t cap = 1024;
                while (cap < list.size()) cap <<= 1;
                e = hipHostMalloc((void **)&b->stage[si], cap * sizeof(RebindItem), hipHostMallocMapped);
                if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&b->stage_dev[si], b->stage[si], 0);
                if (e != hipSuccess) { if (b->stage[si]) (void)hipHostFree(b->stage[si]); b->stage[si] = nullptr; return hip_fail(e, "rebind: pinned item list"); }
                b->stage_cap[si] = cap;
            }
            memcpy(b->stage[si], list.data(), list.size() * sizeof(RebindItem));
            list_dev = b->stage_dev[si];
        } else if (!scatter) {
            si = 2;
            if ((e = await_stage(si)) != hipSuccess) return hip_fail(e, "rebind: waiting for the twin's last copy");
            if (!b->twin_rewritten && K.recorded && (e = hipEventSynchronize(K.ev)) != hipSuccess) return hip_fail(e, "rebind: waiting for the twin's first copy");
            memcpy(K.host, b->h_ticks.data(), sizeof(DTick) * b->h_ticks.size());
            if (!b->h_layers.empty()) memcpy(K.host + b->lo, b->h_layers.data(), sizeof(DLayer) * b->h_layers.size());
            if (split) memcpy(K.host + b->t2o, b->h_ticks2.data(), sizeof(DTick) * b->h_ticks2.size());
            apply((DTick *)K.host, (DLayer *)(K.host + b->lo), split ? (DTick *)(K.host + b->t2o) : nullptr);
            b->twin_rewritten = true;
        }
        // behind every run issued so far, on whatever stream (the block's event), and in front of every run to come
        if (K.last != c->stream) HIP_TRY(hipStreamWaitEvent(c->stream, K.ev, 0));
        if (scatter) e = launcher(K.dev, list.data(), list_dev, (int)list.size(), c->stream);
        else e = hipMemcpyAsync(K.dev, K.host, b->used, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { (void)hipGetLastError(); return hip_fail(e, scatter ? "batch_rebind_scatter" : "descriptors of a batch (rebind)"); }
        if (hipEventRecord(K.ev, c->stream) == hipSuccess) { K.last = c->stream; K.recorded = true; }
        else {
            // no marker behind the operation: nothing may overtake it
            (void)hipGetLastError();
            (void)hipStreamSynchronize(c->stream);
        }
        if (si >= 0) {
            if (hipEventRecord(b->stage_ev[si], c->stream) == hipSuccess) b->stage_pending[si] = true;
            else { (void)hipGetLastError(); (void)hipStreamSynchronize(c->stream); }
            if (si < 2) b->next_stage = si ^ 1;
        }
    }
    // ---- the device has (or will have, in stream order) the new addresses: the host side follows
    apply(b->h_ticks.data(), b->h_layers.data(), split ? b->h_ticks2.data() : nullptr);
    for (const NewPlane &n : np) b->slot_bufs[(size_t)n.slot * 3 + (size_t)n.p] = n.buf;
    // the buffers a run waits for are those bound NOW (one rebound away may be freed by its owner: it is not touched again)
    {
        DepScope scope;
        scope.bufs.reserve(b->slot_bufs.size());
        for (chv_buffer *q : b->slot_bufs) if (q) scope.bufs.push_back(q);
        b->deps = scope.deps();
    }
    return CHV_OK;
}

extern "C" int chv_batch_destroy(chv_batch *b) {
    if (!b) return fail(CHV_ERR_INVALID_VALUE, "null batch");
    (void)hipSetDevice(b->device);
    if (b->blk.dev) desc_block_release(b->device, b->blk);           // (back to the pool: whoever takes it next waits for its event)
    else {
        (void)hipFree(b->d_ticks);
        (void)hipFree(b->d_layers);
        if (b->d_ticks2) (void)hipFree(b->d_ticks2);
    }
    geom_cache_release(b->geom);
    // (a rebind's launch may still be reading a pinned list: its event first)
    for (int i = 0; i < 3; i++) {
        if (b->stage_ev[i]) { if (b->stage_pending[i]) (void)hipEventSynchronize(b->stage_ev[i]); (void)hipEventDestroy(b->stage_ev[i]); }
        if (i < 2 && b->stage[i]) (void)hipHostFree(b->stage[i]);
    }
    b->d_ticks = nullptr;
    delete b;
    return CHV_OK;
}

extern "C" int chv_batch_describe(chv_batch *b, char *kernel_name, size_t cap, int *n_launches) {
    if (!b) return fail(CHV_ERR_INVALID_VALUE, "null batch");
    if (kernel_name && cap) snprintf(kernel_name, cap, "%s", b->kernel_name.c_str());
    if (n_launches) *n_launches = b->fast_path2 != -2 ? 2 : 1;
    return CHV_OK;
}

// ---------------------------------------------------------------------------
// Lanczos-3: tables in double on the host, resampling on the GPU
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// custom kernels (compute.swift:72-73, compute.cl.swift:153-232) through hipRTC
// ---------------------------------------------------------------------------
static const char kCustomPrelude[] = R"CHV(
// ---- CHIPVideo custom-kernel prelude (prefixed to every source given to chv_kernel_build) ----
typedef unsigned char uint8_t;
typedef int int32_t;
typedef unsigned int uint32_t;
struct chv_dev_plane { uint8_t *ptr; int32_t width, height, pitch, components; };
struct chv_dev_image { chv_dev_plane planes[3]; int32_t n_planes, format; };
struct chv_custom_args {
    chv_dev_image target, current;
    chv_dev_image inputs[4];
    int32_t n_inputs, uniforms_size;
    uint8_t uniforms[256];
};
// ImageUniforms, compute.swift:76-86 (236 bytes); each matrix holds the rows of M^-1
struct ImageUniforms {
    float transform[16], textureTransform[16], borderMatrix[16];
    float fillColor[4], inputSize[2], outputSize[2];
    float opacity, imageTime, targetTime;
};
#define CHV_GID_X ((int)(blockIdx.x * blockDim.x + threadIdx.x))
#define CHV_GID_Y ((int)(blockIdx.y * blockDim.y + threadIdx.y))
// the launch is rounded up to 16x16 blocks: leave when outside plane `p`
#define CHV_GUARD(p) do { if (CHV_GID_X >= (p).width || CHV_GID_Y >= (p).height) return; } while (0)
// vecmat4, kernels.cl.swift:27: (dot(v, row0), dot(v, row1), dot(v, row2), dot(v, row3))
__device__ inline float4 chv_vecmat4(float4 v, const float *m) {
    return make_float4(((v.x * m[0] + v.y * m[1]) + v.z * m[2]) + v.w * m[3], ((v.x * m[4] + v.y * m[5]) + v.z * m[6]) + v.w * m[7],
                       ((v.x * m[8] + v.y * m[9]) + v.z * m[10]) + v.w * m[11], ((v.x * m[12] + v.y * m[13]) + v.z * m[14]) + v.w * m[15]);
}
// UNORM_INT8 conversions of OpenCL 1.2 section 8.3.1.1
__device__ inline float chv_unorm8(uint8_t c) { return (float)c / 255.0f; }
__device__ inline uint8_t chv_to_unorm8(float f) {
    float v = rintf(f * 255.0f);
    return (uint8_t)fminf(fmaxf(v, 0.0f), 255.0f);         // NaN -> 0
}
// read_imagef, nearest, unnormalized integer coordinates (zero outside the plane)
__device__ inline float chv_read(const chv_dev_plane &p, int x, int y, int c) {
    if (x < 0 || y < 0 || x >= p.width || y >= p.height) return 0.0f;
    return chv_unorm8(p.ptr[(size_t)y * p.pitch + (size_t)x * p.components + c]);
}
// write_imagef of one component (dropped outside the plane)
__device__ inline void chv_write(const chv_dev_plane &p, int x, int y, int c, float f) {
    if (x < 0 || y < 0 || x >= p.width || y >= p.height) return;
    p.ptr[(size_t)y * p.pitch + (size_t)x * p.components + c] = chv_to_unorm8(f);
}
// read_imagef, LINEAR | CLAMP_TO_EDGE | NORMALIZED (OpenCL 1.2 section 8.2), component c
__device__ inline float chv_sample(const chv_dev_plane &p, float u, float v, int c) {
    float um = u * (float)p.width - 0.5f, vm = v * (float)p.height - 0.5f;
    float fu = floorf(um), fv = floorf(vm);
    float a = um - fu, b = vm - fv;
    int i0 = min(max((int)fu, 0), p.width - 1), i1 = min(max((int)fu + 1, 0), p.width - 1);
    int j0 = min(max((int)fv, 0), p.height - 1), j1 = min(max((int)fv + 1, 0), p.height - 1);
    const uint8_t *r0 = p.ptr + (size_t)j0 * p.pitch + c, *r1 = p.ptr + (size_t)j1 * p.pitch + c;
    float t00 = chv_unorm8(r0[i0 * p.components]), t10 = chv_unorm8(r0[i1 * p.components]);
    float t01 = chv_unorm8(r1[i0 * p.components]), t11 = chv_unorm8(r1[i1 * p.components]);
    return (((1.0f - a) * (1.0f - b) * t00 + a * (1.0f - b) * t10) + (1.0f - a) * b * t01) + a * b * t11;
}
// ---- end of prelude ----
#line 1 "custom_kernel"
)CHV";

extern "C" const char *chv_custom_prelude(void) { return kCustomPrelude; }

extern "C" int chv_kernel_build(chv_context *c, const char *name, const char *source) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (!name || !*name || !source) return fail(CHV_ERR_INVALID_VALUE, "null kernel name or source");
    (void)hipSetDevice(c->device);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    std::string text = std::string(kCustomPrelude) + source;
    hiprtcProgram prog = nullptr;
    if (hiprtcCreateProgram(&prog, text.c_str(), name, 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        return fail(CHV_ERR_UNKNOWN, "hiprtcCreateProgram failed");
    std::string arch = std::string("--offload-arch=") + prop.gcnArchName;
    const char *opts[] = { arch.c_str(), "-O3", "-ffp-contract=off", "-std=c++17" };
    hiprtcResult cr = hiprtcCompileProgram(prog, 4, opts);
    if (cr != HIPRTC_SUCCESS) {
        size_t n = 0;
        std::string log;
        if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) { log.resize(n); (void)hiprtcGetProgramLog(prog, &log[0]); }
        (void)hiprtcDestroyProgram(&prog);
        if (log.size() > 3000) log.resize(3000);
        return fail(CHV_ERR_BAD_INPUT, "Unable to create kernel named %s (%s)\nBuild log:\n%s", name, hiprtcGetErrorString(cr), log.c_str());
    }
    size_t code_size = 0;
    std::vector<char> code;
    if (hiprtcGetCodeSize(prog, &code_size) != HIPRTC_SUCCESS || code_size == 0) { (void)hiprtcDestroyProgram(&prog); return fail(CHV_ERR_UNKNOWN, "hiprtcGetCodeSize failed"); }
    code.resize(code_size);
    hiprtcResult gr = hiprtcGetCode(prog, code.data());
    (void)hiprtcDestroyProgram(&prog);
    if (gr != HIPRTC_SUCCESS) return fail(CHV_ERR_UNKNOWN, "hiprtcGetCode failed");
    auto k = std::make_shared<CustomKernel>();
    k->device = c->device;
    hipError_t e = hipModuleLoadData(&k->module, code.data());
    if (e != hipSuccess) return hip_fail(e, "hipModuleLoadData");
    e = hipModuleGetFunction(&k->fn, k->module, name);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(CHV_ERR_BAD_INPUT, "Unable to create kernel named %s: the source defines no extern \"C\" __global__ function of that name", name);
    }
    c->library[name] = std::move(k);     // merging { $1 }: the new kernel replaces an older one (compute.cl.swift:190-194)
    return CHV_OK;
}

static int image_to_device_any(const chv_image *img, int device, chv_dev_image *out, int err, const char *what) {
    memset(out, 0, sizeof *out);
    if (!img) return fail(err, "null %s image", what);
    if (img->n_planes < 1 || img->n_planes > 3) return fail(err, "%s image has %d planes", what, img->n_planes);
    for (int i = 0; i < img->n_planes; i++) {
        const chv_plane &p = img->planes[i];
        if (p.components != 1 && p.components != 2 && p.components != 4) return fail(err, "%s plane %d: %d components", what, i, p.components);
        DPlane d;
        int rc = plane_to_device(p, p.components, device, &d, err, what, i);
        if (rc) return rc;
        out->planes[i].ptr = d.ptr; out->planes[i].width = d.w; out->planes[i].height = d.h;
        out->planes[i].pitch = d.pitch; out->planes[i].components = d.comps;
    }
    out->n_planes = img->n_planes;
    out->format = img->format;
    return CHV_OK;
}

extern "C" int chv_run_custom(chv_context *c, const char *name, const chv_image *target,
                              const chv_image *inputs, int n_inputs,
                              const void *uniforms, size_t uniforms_size, int blends) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (!name) return fail(CHV_ERR_INVALID_VALUE, "null kernel name");
    auto it = c->library.find(name);
    if (it == c->library.end()) return fail(CHV_ERR_KERNEL_NOT_FOUND, "no custom kernel named %s in this context's library", name);
    if (n_inputs < 0 || n_inputs > CHV_CUSTOM_MAX_INPUTS) return fail(CHV_ERR_BAD_INPUT, "%d input images (max %d)", n_inputs, CHV_CUSTOM_MAX_INPUTS);
    if (n_inputs > 0 && !inputs) return fail(CHV_ERR_BAD_INPUT, "null inputs");
    if (uniforms_size > CHV_CUSTOM_MAX_UNIFORMS || (uniforms_size && !uniforms))
        return fail(CHV_ERR_INVALID_VALUE, "%zu uniform bytes (max %d)", uniforms_size, CHV_CUSTOM_MAX_UNIFORMS);
    (void)hipSetDevice(c->device);
    chv_custom_args a;
    memset(&a, 0, sizeof a);
    DepScope deps;
    int rc = image_to_device_any(target, c->device, &a.target, CHV_ERR_BAD_TARGET, "target");
    if (rc) return rc;
    if (blends) a.current = a.target;
    for (int i = 0; i < n_inputs; i++) {
        rc = image_to_device_any(&inputs[i], c->device, &a.inputs[i], CHV_ERR_BAD_INPUT, "input");
        if (rc) return rc;
    }
    a.n_inputs = n_inputs;
    a.uniforms_size = (int32_t)uniforms_size;
    if (uniforms_size) memcpy(a.uniforms, uniforms, uniforms_size);
    auto dp = deps.deps();
    rc = wait_for_uploads(c->stream, dp);
    if (rc) return rc;
    size_t size = sizeof a;
    void *config[] = { HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END };
    const unsigned gx = (unsigned)(a.target.planes[0].width + 15) / 16, gy = (unsigned)(a.target.planes[0].height + 15) / 16;
    HIP_TRY(hipModuleLaunchKernel(it->second->fn, gx, gy, 1, 16, 16, 1, 0, c->stream, nullptr, config));
    return CHV_OK;
}

static double sinc_pi(double t) {
    if (t == 0.0) return 1.0;
    double pt = 3.14159265358979323846 * t;
    return std::sin(pt) / pt;
}

static int lanczos_host_table(int in_size, int out_size, int *taps_out, std::vector<int32_t> *first,
                              std::vector<float> *weights) {
    double scale = (double)in_size / (double)out_size;
    double fs = scale > 1.0 ? scale : 1.0;
    double support = 3.0 * fs;
    int taps = 2 * (int)std::ceil(support);
    if (taps > 256) return fail(CHV_ERR_INVALID_VALUE, "Lanczos ratio %d:%d needs %d taps (max 256)", in_size, out_size, taps);
    first->resize(out_size);
    weights->resize((size_t)out_size * taps);
    std::vector<double> w(taps);
    for (int o = 0; o < out_size; o++) {
        double center = ((double)o + 0.5) * scale - 0.5;
        int f = (int)std::floor(center - support) + 1;
        double sum = 0.0;
        for (int k = 0; k < taps; k++) {
            double t = ((double)(f + k) - center) / fs;
            double v = (t > -3.0 && t < 3.0) ? sinc_pi(t) * sinc_pi(t / 3.0) : 0.0;
            w[k] = v;
            sum += v;
        }
        (*first)[o] = f;
        for (int k = 0; k < taps; k++) (*weights)[(size_t)o * taps + k] = (float)(w[k] / sum);
    }
    *taps_out = taps;
    return CHV_OK;
}

static int lanczos_table(chv_context *c, int in_size, int out_size, LanczosRef *out) {
    DeviceShared &sh = *c->shared;
    auto key = std::make_pair(in_size, out_size);
    {
        std::lock_guard<std::mutex> lock(sh.mu);
        auto it = sh.lanczos.find(key);
        if (it != sh.lanczos.end()) { it->second.last_use = ++sh.lanczos_clock; *out = it->second.tab; return CHV_OK; }
    }
    // build and upload outside the lock: other contexts of the device keep running meanwhile
    std::vector<int32_t> first;
    std::vector<float> weights;
    LanczosRef t = std::make_shared<LanczosTable>();
    t->device = c->device;
    int rc = lanczos_host_table(in_size, out_size, &t->taps, &first, &weights);
    if (rc) return rc;
    t->first0 = first[0];
    t->stride = first.size() > 1 ? first[1] - first[0] : 0;
    for (size_t o = 1; o + 1 < first.size() && t->stride; o++) if (first[o + 1] - first[o] != t->stride) t->stride = 0;
    HIP_TRY(hipMalloc((void **)&t->first, first.size() * sizeof(int32_t)));
    hipError_t e = hipMalloc((void **)&t->weights, weights.size() * sizeof(float));
    if (e != hipSuccess) t->weights = nullptr;
    if (e == hipSuccess)
        e = hipMemcpy(t->first, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(t->weights, weights.data(), weights.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "lanczos table upload");     // (t frees what it holds)
    // Evicted tables are parked and freed kLanczosRetireBatch at a time — an animated resize makes a new (in, out) pair per
    // frame, and one hipFree per miss would put a device-wide synchronisation into every tick.  Only tables nobody else
    // holds are freed: a context between its lookup and its launch keeps its reference, and the table with it.
    std::vector<LanczosRef> to_free;
    {
        std::lock_guard<std::mutex> lock(sh.mu);
        auto it = sh.lanczos.find(key);
        if (it != sh.lanczos.end()) {                       // another context built the same table meanwhile: keep theirs
            it->second.last_use = ++sh.lanczos_clock;
            *out = it->second.tab;
            to_free.push_back(std::move(t));
        } else {
            if (sh.lanczos.size() >= kLanczosCacheEntries) {
                auto lru = sh.lanczos.begin();
                for (auto jt = sh.lanczos.begin(); jt != sh.lanczos.end(); ++jt) if (jt->second.last_use < lru->second.last_use) lru = jt;
                sh.lanczos_retired.push_back(std::move(lru->second.tab));
                sh.lanczos.erase(lru);
            }
            LanczosEntry en;
            en.tab = t; en.last_use = ++sh.lanczos_clock;
            sh.lanczos[key] = en;
            *out = std::move(t);
            if (sh.lanczos_retired.size() >= kLanczosRetireBatch) {
                std::vector<LanczosRef> keep;
                for (LanczosRef &r : sh.lanczos_retired) (r.use_count() == 1 ? to_free : keep).push_back(std::move(r));
                sh.lanczos_retired.swap(keep);
            }
        }
    }
    to_free.clear();      // outside the lock: ~LanczosTable -> hipFree, which waits for queued work that may still read the tables
    return CHV_OK;
}

// ---- the common host path of the Lanczos entries ----
// Pictures per descriptor slot: the plane records of one picture — its targets rung by rung, then its source planes once — must fit one
// slot together, and a chunk is what fits one.  include/chipvideo.h states the same rule per entry (the CHV_*_CHUNK macros and the counts).
static constexpr int lanczos_chunk(size_t records_per_picture) { return (int)(kDescSlotBytes / (records_per_picture * sizeof(DPlane))); }
static_assert(CHV_LADDER_SLOT_BYTES == kDescSlotBytes && CHV_LADDER_PLANE_BYTES == sizeof(DPlane), "include/chipvideo.h states the descriptor slot and the plane record");

// The launch prologue, after a call's validation: a build without the entry's launcher refuses (`missing` is that refusal, CHV_OK with a
// launcher: `launcher ? CHV_OK : fail(...)` keeps the message at the entry), then the device and the uploads the planes wait for.
static int lanczos_begin(chv_context *c, const DepScope &deps, int missing) {
    if (missing) return missing;
    HIP_TRY(hipSetDevice(c->device));
    auto dp = deps.deps();
    return wait_for_uploads(c->stream, dp);
}

// The tables of one plane: (src_w, dst_w), then (src_h, dst_h) — the order the shared cache sees.  The caller owns *rx and *ry and holds
// them until the last launch of the call is enqueued.
static int lanczos_table_pair(chv_context *c, int src_w, int src_h, int dst_w, int dst_h, LanczosRef *rx, LanczosRef *ry, LanczosPlaneTables *out) {
    int rc = lanczos_table(c, src_w, dst_w, rx);
    if (rc) return rc;
    rc = lanczos_table(c, src_h, dst_h, ry);
    if (rc) return rc;
    *out = LanczosPlaneTables{ (*rx)->first, (*rx)->weights, (*ry)->first, (*ry)->weights, (*rx)->taps, (*ry)->taps };
    return CHV_OK;
}

// n pictures of `per` records each leave through the pinned, device-mapped descriptor ring, per_slot pictures to a chunk: a longer list is
// split along the PICTURES, so all records of a picture leave together.  A DescSlot lives exactly for one chunk's launch; the sticky error
// is cleared right before launch(dev, m), which sets the job's batch and n_pictures, launches, counts, and returns the entry's status.
template <class Launch>
static int lanczos_send(chv_context *c, const DPlane *records, size_t per, int n, int per_slot, Launch launch) {
    for (int first = 0; first < n; first += per_slot) {
        const int m = std::min(per_slot, n - first);
        DescSlot ds(c);
        if (ds.rc) return ds.rc;
        DPlane *host = (DPlane *)(c->desc_host + (size_t)ds.slot * kDescSlotBytes);
        memcpy(host, records + per * first, sizeof(DPlane) * per * (size_t)m);
        DPlane *dev = nullptr;
        HIP_TRY(hipHostGetDevicePointer((void **)&dev, host, 0));
        (void)hipGetLastError();
        int rc = launch(dev, m);
        if (rc) return rc;
    }
    return CHV_OK;
}

// The head of every ladder entry: the list's shape.  *empty: a ladder of no rungs or no sources, which is CHV_OK and does nothing.
static int lanczos_ladder_header(const chv_image *dsts, int n_rungs, const chv_image *srcs, int n, bool *empty) {
    *empty = false;
    if (n_rungs < 0 || n_rungs > CHV_LADDER_MAX_RUNGS) return fail(CHV_ERR_INVALID_VALUE, "a ladder has 0 to %d rungs, not %d", CHV_LADDER_MAX_RUNGS, n_rungs);
    if (n < 0) return fail(CHV_ERR_INVALID_VALUE, "bad ladder: %d sources", n);
    if (n_rungs == 0 || n == 0) { *empty = true; return CHV_OK; }
    if (!dsts || !srcs) return fail(CHV_ERR_INVALID_VALUE, "bad ladder: a null list");
    return CHV_OK;
}

// One target format and one source format per ladder: the list's mistake, not the image's — before anything else of the images is looked at.
static int lanczos_ladder_formats(const chv_image *dsts, int n_rungs, const chv_image *srcs, int n) {
    for (int k = 1; k < n_rungs * n; k++)
        if (dsts[k].format != dsts[0].format)
            return fail(CHV_ERR_INVALID_VALUE, "rung %d, target %d has format %d, the ladder began with %d (one target format per ladder)", k / n, k % n, dsts[k].format, dsts[0].format);
    for (int i = 1; i < n; i++)
        if (srcs[i].format != srcs[0].format)
            return fail(CHV_ERR_INVALID_VALUE, "source %d has format %d, the ladder began with %d (one source format per ladder)", i, srcs[i].format, srcs[0].format);
    return CHV_OK;
}

// the snp planes of source i have the sizes of the ladder's first source
static int lanczos_one_source_size(const DPlane *src, const DPlane *first, int snp, int i) {
    for (int p = 0; p < snp; p++)
        if (src[p].w != first[p].w || src[p].h != first[p].h)
            return fail(CHV_ERR_INVALID_VALUE, "source %d, plane %d is %dx%d, the ladder began with %dx%d (one source size per ladder)", i, p, src[p].w, src[p].h,
                        first[p].w, first[p].h);
    return CHV_OK;
}

// ---- the 4:2:0 families of chv_scale_lanczos: NV12 (planes of 1 and 2 components) and y420p (three planes of 1), plane by plane ----
// Pictures per descriptor slot of a batch chunk: a picture's np plane pairs, lanczos_chunk(2 * np).
static_assert(lanczos_chunk(4) == 62 && lanczos_chunk(6) == 41, "include/chipvideo.h states the counts");
static_assert(lanczos_chunk(4) <= CHV_LANCZOS_BATCH_CHUNK && lanczos_chunk(6) <= CHV_LANCZOS_BATCH_CHUNK, "no planar chunk is longer than a BGRA one");

// planes of a 4:2:0 Lanczos family, 0 for every other (format, structure)
static int lanczos_planar_planes(const chv_image *img) {
    if (!img) return 0;
    if (img->format == CHV_FMT_NV12 && img->n_planes == 2) return 2;
    if (img->format == CHV_FMT_Y420P && img->n_planes == 3) return 3;
    return 0;
}
static int lanczos_planar_comps(int format, int plane) { return format == CHV_FMT_NV12 && plane == 1 ? 2 : 1; }

// (dst, src) of one picture -> np plane pairs at out[2 p], out[2 p + 1]; every check of plane_to_device on every plane
static int lanczos_planar_pairs(chv_context *c, const chv_image *dst, const chv_image *src, int np, int idx, DPlane *out) {
    if (lanczos_planar_planes(src) != np || src->format != dst->format)
        return fail(CHV_ERR_BAD_INPUT, "Lanczos source %d must have the target's format and planes (%s, %d planes)", idx, dst->format == CHV_FMT_NV12 ? "nv12" : "y420p", np);
    for (int p = 0; p < np; p++) {
        const int comps = lanczos_planar_comps(dst->format, p);
        int rc = plane_to_device(dst->planes[p], comps, c->device, &out[2 * p], CHV_ERR_BAD_TARGET, "target", p);
        if (rc) return rc;
        rc = plane_to_device(src->planes[p], comps, c->device, &out[2 * p + 1], CHV_ERR_BAD_INPUT, "input", p);
        if (rc) return rc;
    }
    return CHV_OK;
}

// the tables of every plane of one geometry (up to four distinct ones; the references are held until the launch is enqueued)
static int lanczos_planar_job(chv_context *c, const DPlane *pairs, int np, LanczosRef *refs, LanczosPlanarJob *job) {
    memset(job, 0, sizeof *job);
    job->n_planes = np;
    for (int p = 0; p < np; p++) {
        const DPlane &d = pairs[2 * p], &s = pairs[2 * p + 1];
        int rc = lanczos_table_pair(c, s.w, s.h, d.w, d.h, &refs[2 * p], &refs[2 * p + 1], &job->tab[p]);
        if (rc) return rc;
        job->dst[p] = d; job->src[p] = s;
    }
    return CHV_OK;
}

static int scale_lanczos_planar(chv_context *c, const chv_image *dst, const chv_image *src, int np) {
    const LanczosPlanarLauncher launcher = g_lanczos_planar_launcher.load(std::memory_order_acquire);
    DPlane pairs[2 * kLanczosPlanarMaxPlanes];
    DepScope deps;
    int rc = lanczos_planar_pairs(c, dst, src, np, 0, pairs);
    if (rc) return rc;
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no planar Lanczos kernels"));
    if (rc) return rc;
    LanczosRef refs[2 * kLanczosPlanarMaxPlanes];
    LanczosPlanarJob job;
    rc = lanczos_planar_job(c, pairs, np, refs, &job);
    if (rc) return rc;
    job.batch = nullptr; job.n_pictures = 1;
    (void)hipGetLastError();
    hipError_t e = launcher(job, c->stream);
    if (e != hipSuccess) return hip_fail(e, "lanczos launch");
    return CHV_OK;
}

static int scale_lanczos_planar_batch(chv_context *c, const chv_image *dsts, const chv_image *srcs, int n, int np) {
    const LanczosPlanarLauncher launcher = g_lanczos_planar_launcher.load(std::memory_order_acquire);
    std::vector<DPlane> pairs((size_t)2 * np * n);
    DepScope deps;
    for (int i = 0; i < n; i++) {
        if (dsts[i].format != dsts[0].format || lanczos_planar_planes(&dsts[i]) != np)
            return fail(CHV_ERR_INVALID_VALUE, "target %d: format %d with %d planes, the batch is format %d with %d planes (one format per batch)", i,
                        dsts[i].format, dsts[i].n_planes, dsts[0].format, np);
        if (srcs[i].format != dsts[0].format || lanczos_planar_planes(&srcs[i]) != np)
            return fail(CHV_ERR_INVALID_VALUE, "source %d: format %d with %d planes, the batch is format %d with %d planes (one format per batch)", i,
                        srcs[i].format, srcs[i].n_planes, dsts[0].format, np);
        DPlane *pi = pairs.data() + (size_t)2 * np * i;
        int rc = lanczos_planar_pairs(c, &dsts[i], &srcs[i], np, i, pi);
        if (rc) return rc;
        for (int q = 0; q < 2 * np; q++)
            if (pi[q].w != pairs[q].w || pi[q].h != pairs[q].h)
                return fail(CHV_ERR_INVALID_VALUE, "pair %d, plane %d: %dx%d -> %dx%d, the batch is %dx%d -> %dx%d (one geometry per batch)", i, q / 2,
                            pi[q | 1].w, pi[q | 1].h, pi[q & ~1].w, pi[q & ~1].h, pairs[q | 1].w, pairs[q | 1].h, pairs[q & ~1].w, pairs[q & ~1].h);
    }
    int rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no planar Lanczos kernels"));
    if (rc) return rc;
    LanczosRef refs[2 * kLanczosPlanarMaxPlanes];
    LanczosPlanarJob job;
    rc = lanczos_planar_job(c, pairs.data(), np, refs, &job);
    if (rc) return rc;
    const size_t per = (size_t)2 * np;
    return lanczos_send(c, pairs.data(), per, n, lanczos_chunk(per), [&](DPlane *dev, int m) {
        job.batch = dev; job.n_pictures = m;
        hipError_t e = launcher(job, c->stream);
        return e != hipSuccess ? hip_fail(e, "lanczos launch") : CHV_OK;
    });
}

extern "C" int chv_scale_lanczos(chv_context *c, const chv_image *dst, const chv_image *src) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (const int np = lanczos_planar_planes(dst)) return scale_lanczos_planar(c, dst, src, np);
    if (dst && (dst->format == CHV_FMT_NV12 || dst->format == CHV_FMT_Y420P))
        return fail(CHV_ERR_BAD_TARGET, "Lanczos target: a %s image has %d planes, not %d", dst->format == CHV_FMT_NV12 ? "nv12" : "y420p",
                    dst->format == CHV_FMT_NV12 ? 2 : 3, dst->n_planes);
    if (!dst || dst->n_planes != 1) return fail(CHV_ERR_BAD_TARGET, "Lanczos target must be one 4-component plane");
    if (!src || src->n_planes != 1) return fail(CHV_ERR_BAD_INPUT, "Lanczos source must be one 4-component plane");
    DPlane d, s;
    DepScope deps;
    int rc = plane_to_device(dst->planes[0], 4, c->device, &d, CHV_ERR_BAD_TARGET, "target", 0);
    if (rc) return rc;
    rc = plane_to_device(src->planes[0], 4, c->device, &s, CHV_ERR_BAD_INPUT, "input", 0);
    if (rc) return rc;
    rc = lanczos_begin(c, deps, CHV_OK);      // (the 4-component kernels are part of every build)
    if (rc) return rc;
    LanczosRef tx, ty;      // held until the launch is enqueued (see LanczosTable)
    LanczosPlaneTables t;
    rc = lanczos_table_pair(c, s.w, s.h, d.w, d.h, &tx, &ty, &t);
    if (rc) return rc;
    (void)hipGetLastError();
    hipError_t e = launch_lanczos(d, s, t.fx, t.wx, t.tx, t.fy, t.wy, t.ty, c->stream, nullptr, 0, tx->stride, tx->first0, ty->stride);
    if (e != hipSuccess) return hip_fail(e, "lanczos launch");
    return CHV_OK;
}

// Many resizes of ONE geometry (all sources of one size, all targets of one size) in one launch per chunk: what a host with
// several streams per device issues per tick (a 2160p -> 1080p pass is 28 us of device time, of the order of a launch).
extern "C" int chv_scale_lanczos_batch(chv_context *c, const chv_image *dsts, const chv_image *srcs, int n) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (n <= 0 || !dsts || !srcs) return fail(CHV_ERR_INVALID_VALUE, "empty batch");
    if (const int np = lanczos_planar_planes(&dsts[0])) return scale_lanczos_planar_batch(c, dsts, srcs, n, np);
    std::vector<DPlane> pairs((size_t)2 * n);
    DepScope deps;
    // (one format per batch: a 4:2:0 picture among 4-component planes is the list's mistake, not the image's — before anything else is looked at)
    for (int i = 1; i < n; i++)
        if (lanczos_planar_planes(&dsts[i]) || lanczos_planar_planes(&srcs[i]))
            return fail(CHV_ERR_INVALID_VALUE, "pair %d is a 4:2:0 picture, the batch began with a 4-component plane (one format per batch)", i);
    for (int i = 0; i < n; i++) {
        if (dsts[i].n_planes != 1) return fail(CHV_ERR_BAD_TARGET, "Lanczos target %d must be one 4-component plane", i);
        if (srcs[i].n_planes != 1) return fail(CHV_ERR_BAD_INPUT, "Lanczos source %d must be one 4-component plane", i);
        int rc = plane_to_device(dsts[i].planes[0], 4, c->device, &pairs[2 * i], CHV_ERR_BAD_TARGET, "target", i);
        if (rc) return rc;
        rc = plane_to_device(srcs[i].planes[0], 4, c->device, &pairs[2 * i + 1], CHV_ERR_BAD_INPUT, "input", i);
        if (rc) return rc;
        if (pairs[2 * i].w != pairs[0].w || pairs[2 * i].h != pairs[0].h || pairs[2 * i + 1].w != pairs[1].w || pairs[2 * i + 1].h != pairs[1].h)
            return fail(CHV_ERR_INVALID_VALUE, "pair %d: %dx%d -> %dx%d, the batch is %dx%d -> %dx%d (one geometry per batch)", i,
                        pairs[2 * i + 1].w, pairs[2 * i + 1].h, pairs[2 * i].w, pairs[2 * i].h, pairs[1].w, pairs[1].h, pairs[0].w, pairs[0].h);
    }
    int rc = lanczos_begin(c, deps, CHV_OK);
    if (rc) return rc;
    LanczosRef tx, ty;
    LanczosPlaneTables t;
    rc = lanczos_table_pair(c, pairs[1].w, pairs[1].h, pairs[0].w, pairs[0].h, &tx, &ty, &t);
    if (rc) return rc;
    // (the ABI's chunk of 64 pairs is shorter than what a slot holds)
    static_assert(CHV_LANCZOS_BATCH_CHUNK <= lanczos_chunk(2), "a chunk's plane pairs must fit one descriptor slot");
    return lanczos_send(c, pairs.data(), 2, n, CHV_LANCZOS_BATCH_CHUNK, [&](DPlane *dev, int m) {
        hipError_t e = launch_lanczos(pairs[0], pairs[1], t.fx, t.wx, t.tx, t.fy, t.wy, t.ty, c->stream, dev, m, tx->stride, tx->first0, ty->stride);
        return e != hipSuccess ? hip_fail(e, "lanczos launch") : CHV_OK;
    });
}

// ---- chv_scale_lanczos_to_yuv: one BGRA / RGBA plane -> an NV12 or y420p picture ----
// Pictures per descriptor slot of a batch chunk: a picture's np target planes and its source plane, lanczos_chunk(np + 1).
static_assert(lanczos_chunk(3) == 83 && lanczos_chunk(4) == 62, "a chunk is what fits one descriptor slot (include/chipvideo.h states the counts)");

// DESIGN.md section 4.5's table (the device's copy is kR2Y, pixel_math.hip.h): yoff, then the y, u and v rows over (R, G, B)
static const int32_t kR2YHost[4][10] = {
    { 16, 16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681 },   // BT.601 limited
    { 16, 11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639 },   // BT.709 limited
    { 0, 19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329 },   // BT.601 full
    { 0, 13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005 },    // BT.709 full
};

// (dst, src) of one picture -> its np target planes at out[0 .. np - 1], its source plane at out[np]; every check of plane_to_device
static int lanczos_to_yuv_planes(chv_context *c, const chv_image *dst, const chv_image *src, int idx, DPlane *out) {
    const int np = lanczos_planar_planes(dst);
    if (!np) return fail(CHV_ERR_BAD_TARGET, "Lanczos to YUV: target %d must be nv12 with 2 planes or y420p with 3", idx);
    if (!src || src->n_planes != 1 || (src->format != CHV_FMT_BGRA && src->format != CHV_FMT_RGBA))
        return fail(CHV_ERR_BAD_INPUT, "Lanczos to YUV: source %d must be one 4-component plane of format BGRA or RGBA", idx);
    for (int p = 0; p < np; p++) {
        int rc = plane_to_device(dst->planes[p], lanczos_planar_comps(dst->format, p), c->device, &out[p], CHV_ERR_BAD_TARGET, "target", p);
        if (rc) return rc;
        if (p && (out[p].w != std::max(1, out[0].w / 2) || out[p].h != std::max(1, out[0].h / 2)))
            return fail(CHV_ERR_BAD_TARGET, "Lanczos to YUV: target %d, plane %d is %dx%d, a %dx%d picture's chroma is %dx%d", idx, p, out[p].w, out[p].h,
                        out[0].w, out[0].h, std::max(1, out[0].w / 2), std::max(1, out[0].h / 2));
    }
    return plane_to_device(src->planes[0], 4, c->device, &out[np], CHV_ERR_BAD_INPUT, "input", 0);
}

// section 4.5's rows for `opts` (NULL: BT.601 limited) in the source's BYTE order: the first and third column exchanged for a BGRA source
static void lanczos_to_yuv_matrix(int src_format, const chv_kernel_opts *opts, int32_t *yoff, int32_t ky[3], int32_t ku[3], int32_t kv[3]) {
    const int32_t *k = kR2YHost[(opts ? opts->colorspace : CHV_CSC_BT601_LIMITED) & 3];
    const int r = src_format == CHV_FMT_BGRA ? 2 : 0, b = 2 - r;      // the byte that holds red, blue
    *yoff = k[0];
    ky[r] = k[1]; ky[1] = k[2]; ky[b] = k[3];
    ku[r] = k[4]; ku[1] = k[5]; ku[b] = k[6];
    kv[r] = k[7]; kv[1] = k[8]; kv[b] = k[9];
}

static void lanczos_to_yuv_job(const DPlane *planes, int np, int src_format, const chv_kernel_opts *opts, const LanczosPlaneTables &t, LanczosToYuvJob *job) {
    memset(job, 0, sizeof *job);
    job->fx = t.fx; job->wx = t.wx; job->fy = t.fy; job->wy = t.wy; job->tx = t.tx; job->ty = t.ty;
    job->n_dst = np;
    for (int p = 0; p < np; p++) job->dst[p] = planes[p];
    job->src = planes[np];
    lanczos_to_yuv_matrix(src_format, opts, &job->yoff, job->ky, job->ku, job->kv);
}

extern "C" int chv_scale_lanczos_to_yuv(chv_context *c, const chv_image *dst, const chv_image *src, const chv_kernel_opts *opts) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    const LanczosToYuvLauncher launcher = g_lanczos_to_yuv_launcher.load(std::memory_order_acquire);
    DPlane planes[kLanczosToYuvMaxPlanes + 1];
    DepScope deps;
    int rc = lanczos_to_yuv_planes(c, dst, src, 0, planes);
    if (rc) return rc;
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no Lanczos to YUV kernels"));
    if (rc) return rc;
    const int np = dst->n_planes;
    LanczosRef tx, ty;      // held until the launch is enqueued (see LanczosTable)
    LanczosPlaneTables t;
    rc = lanczos_table_pair(c, planes[np].w, planes[np].h, planes[0].w, planes[0].h, &tx, &ty, &t);
    if (rc) return rc;
    LanczosToYuvJob job;
    lanczos_to_yuv_job(planes, np, src->format, opts, t, &job);
    job.batch = nullptr; job.n_pictures = 1;
    (void)hipGetLastError();
    hipError_t e = launcher(job, c->stream);
    if (e != hipSuccess) return hip_fail(e, "lanczos launch");
    return CHV_OK;
}

extern "C" int chv_scale_lanczos_to_yuv_batch(chv_context *c, const chv_image *dsts, const chv_image *srcs, int n, const chv_kernel_opts *opts) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (n == 0) return CHV_OK;
    if (n < 0 || !dsts || !srcs) return fail(CHV_ERR_INVALID_VALUE, "bad batch");
    const LanczosToYuvLauncher launcher = g_lanczos_to_yuv_launcher.load(std::memory_order_acquire);
    const int np = lanczos_planar_planes(&dsts[0]);
    if (!np) return fail(CHV_ERR_BAD_TARGET, "Lanczos to YUV: target 0 must be nv12 with 2 planes or y420p with 3");
    const size_t per = (size_t)np + 1;
    std::vector<DPlane> planes(per * n);
    DepScope deps;
    // (one target format and one source format per batch: the list's mistake, not the image's — before anything else is looked at)
    for (int i = 1; i < n; i++) {
        if (dsts[i].format != dsts[0].format)
            return fail(CHV_ERR_INVALID_VALUE, "target %d has format %d, the batch began with %d (one target format per batch)", i, dsts[i].format, dsts[0].format);
        if (srcs[i].format != srcs[0].format)
            return fail(CHV_ERR_INVALID_VALUE, "source %d has format %d, the batch began with %d (one source format per batch)", i, srcs[i].format, srcs[0].format);
    }
    for (int i = 0; i < n; i++) {
        DPlane *pi = planes.data() + per * i;
        int rc = lanczos_to_yuv_planes(c, &dsts[i], &srcs[i], i, pi);
        if (rc) return rc;
        if (pi[0].w != planes[0].w || pi[0].h != planes[0].h || pi[np].w != planes[np].w || pi[np].h != planes[np].h)
            return fail(CHV_ERR_INVALID_VALUE, "pair %d: %dx%d -> %dx%d, the batch is %dx%d -> %dx%d (one geometry per batch)", i,
                        pi[np].w, pi[np].h, pi[0].w, pi[0].h, planes[np].w, planes[np].h, planes[0].w, planes[0].h);
    }
    int rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no Lanczos to YUV kernels"));
    if (rc) return rc;
    LanczosRef tx, ty;
    LanczosPlaneTables t;
    rc = lanczos_table_pair(c, planes[np].w, planes[np].h, planes[0].w, planes[0].h, &tx, &ty, &t);
    if (rc) return rc;
    LanczosToYuvJob job;
    lanczos_to_yuv_job(planes.data(), np, srcs[0].format, opts, t, &job);
    return lanczos_send(c, planes.data(), per, n, lanczos_chunk(per), [&](DPlane *dev, int m) {
        job.batch = dev; job.n_pictures = m;
        hipError_t e = launcher(job, c->stream);
        return e != hipSuccess ? hip_fail(e, "lanczos launch") : CHV_OK;
    });
}

// ---- chv_scale_lanczos_to_yuv_ladder: every rung of an encoder ladder in one launch per route ----
// Pictures per descriptor slot of a chunk: a picture's np target planes of every rung and its source plane, lanczos_chunk(n_rungs * np + 1).
// include/chipvideo.h states the rule as CHV_LADDER_CHUNK.
static_assert(CHV_LADDER_MAX_RUNGS == kLanczosLadderMaxRungs, "lanczos_ladder.h carries as many rungs as the ABI admits");
static_assert(CHV_LADDER_CHUNK(1, 2) == lanczos_chunk(3) && CHV_LADDER_CHUNK(1, 3) == lanczos_chunk(4), "a ladder of one rung is chunked like chv_scale_lanczos_to_yuv_batch");
static_assert(lanczos_chunk(CHV_LADDER_MAX_RUNGS * 3 + 1) >= 1 && lanczos_chunk(2 * 2 + 1) == CHV_LADDER_CHUNK(2, 2) && lanczos_chunk(8 * 3 + 1) == CHV_LADDER_CHUNK(8, 3),
              "the longest ladder of the widest format fits one descriptor slot; a chunk is what fits one (include/chipvideo.h states the rule)");

extern "C" int chv_scale_lanczos_to_yuv_ladder(chv_context *c, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n, const chv_kernel_opts *opts) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    bool empty;
    int rc = lanczos_ladder_header(dsts, n_rungs, srcs, n, &empty);
    if (rc || empty) return rc;
    const LanczosLadderLauncher launcher = g_lanczos_ladder_launcher.load(std::memory_order_acquire);
    const int np = lanczos_planar_planes(&dsts[0]);
    if (!np) return fail(CHV_ERR_BAD_TARGET, "Lanczos to YUV: target 0 must be nv12 with 2 planes or y420p with 3");
    rc = lanczos_ladder_formats(dsts, n_rungs, srcs, n);
    if (rc) return rc;
    // a picture's descriptor: the np target planes of rung 0, of rung 1, ..., then the source plane
    const size_t per = (size_t)n_rungs * np + 1;
    std::vector<DPlane> planes(per * n);
    DepScope deps;
    for (int i = 0; i < n; i++) {
        DPlane *pi = planes.data() + per * i;
        for (int r = 0; r < n_rungs; r++) {
            DPlane one[kLanczosToYuvMaxPlanes + 1];
            rc = lanczos_to_yuv_planes(c, &dsts[(size_t)r * n + i], &srcs[i], r * n + i, one);
            if (rc) return rc;
            for (int p = 0; p < np; p++) pi[r * np + p] = one[p];
            pi[per - 1] = one[np];
            if (one[0].w != planes[r * np].w || one[0].h != planes[r * np].h)
                return fail(CHV_ERR_INVALID_VALUE, "rung %d, target %d is %dx%d, the rung began with %dx%d (one size per rung)", r, i, one[0].w, one[0].h,
                            planes[r * np].w, planes[r * np].h);
        }
        if (pi[per - 1].w != planes[per - 1].w || pi[per - 1].h != planes[per - 1].h)
            return fail(CHV_ERR_INVALID_VALUE, "source %d is %dx%d, the ladder began with %dx%d (one source size per ladder)", i, pi[per - 1].w, pi[per - 1].h,
                        planes[per - 1].w, planes[per - 1].h);
    }
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no Lanczos ladder kernels"));
    if (rc) return rc;
    // two tables per rung (rungs of one geometry share theirs)
    LanczosRef refs[2 * CHV_LADDER_MAX_RUNGS];
    LanczosLadderJob job;
    memset(&job, 0, sizeof job);
    job.n_rungs = n_rungs; job.n_dst = np;
    job.src_w = planes[per - 1].w; job.src_h = planes[per - 1].h;
    for (int r = 0; r < n_rungs; r++) {
        const DPlane &d = planes[r * np];
        LanczosPlaneTables t;
        rc = lanczos_table_pair(c, job.src_w, job.src_h, d.w, d.h, &refs[2 * r], &refs[2 * r + 1], &t);
        if (rc) return rc;
        job.rung[r] = LanczosLadderRung{ t.fx, t.wx, t.fy, t.wy, t.tx, t.ty, d.w, d.h };
    }
    lanczos_to_yuv_matrix(srcs[0].format, opts, &job.yoff, job.ky, job.ku, job.kv);
    return lanczos_send(c, planes.data(), per, n, lanczos_chunk(per), [&](DPlane *dev, int m) {
        job.batch = dev; job.n_pictures = m;
        int launches = 0;
        hipError_t e = launcher(job, c->stream, &launches);
        debug_counters().lanczos_ladder_launches.fetch_add((unsigned long long)launches, std::memory_order_relaxed);
        return e != hipSuccess ? hip_fail(e, "lanczos ladder launch") : CHV_OK;
    });
}

// ---- chv_scale_lanczos_ladder: every rung of a 4:2:0 ladder in one launch per route ----
// Pictures per descriptor slot of a chunk: a picture's np target planes of every rung and its np source planes, lanczos_chunk((n_rungs + 1) * np).
// include/chipvideo.h states the rule as CHV_PLANAR_LADDER_CHUNK.
static_assert(CHV_LADDER_MAX_RUNGS == kLanczosPlanarLadderMaxRungs, "lanczos_planar_ladder.h carries as many rungs as the ABI admits");
static_assert(CHV_PLANAR_LADDER_CHUNK(1, 2) == lanczos_chunk(4) && CHV_PLANAR_LADDER_CHUNK(1, 3) == lanczos_chunk(6), "a ladder of one rung is chunked like chv_scale_lanczos_batch");
static_assert(lanczos_chunk((CHV_LADDER_MAX_RUNGS + 1) * 3) >= 1 && lanczos_chunk((2 + 1) * 2) == CHV_PLANAR_LADDER_CHUNK(2, 2) &&
              lanczos_chunk((3 + 1) * 3) == CHV_PLANAR_LADDER_CHUNK(3, 3) && lanczos_chunk((8 + 1) * 3) == CHV_PLANAR_LADDER_CHUNK(8, 3),
              "the longest ladder of the widest format fits one descriptor slot; a chunk is what fits one (include/chipvideo.h states the rule)");

extern "C" int chv_scale_lanczos_ladder(chv_context *c, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    bool empty;
    int rc = lanczos_ladder_header(dsts, n_rungs, srcs, n, &empty);
    if (rc || empty) return rc;
    const LanczosPlanarLadderLauncher launcher = g_lanczos_planar_ladder_launcher.load(std::memory_order_acquire);
    const int np = lanczos_planar_planes(&dsts[0]);
    if (!np) return fail(CHV_ERR_BAD_TARGET, "Lanczos ladder: target 0 must be nv12 with 2 planes or y420p with 3 (there is no 4-component ladder)");
    rc = lanczos_ladder_formats(dsts, n_rungs, srcs, n);
    if (rc) return rc;
    // a picture's record: the np target planes of rung 0, of rung 1, ..., then the np source planes
    const size_t per = (size_t)(n_rungs + 1) * np, src_at = (size_t)n_rungs * np;
    std::vector<DPlane> planes(per * n);
    DepScope deps;
    for (int i = 0; i < n; i++) {
        DPlane *pi = planes.data() + per * i;
        for (int r = 0; r < n_rungs; r++) {
            DPlane pairs[2 * kLanczosPlanarMaxPlanes];
            rc = lanczos_planar_pairs(c, &dsts[(size_t)r * n + i], &srcs[i], np, r * n + i, pairs);
            if (rc) return rc;
            for (int p = 0; p < np; p++) {
                pi[r * np + p] = pairs[2 * p];
                pi[src_at + p] = pairs[2 * p + 1];
                const DPlane &d0 = planes[r * np + p];
                if (pairs[2 * p].w != d0.w || pairs[2 * p].h != d0.h)
                    return fail(CHV_ERR_INVALID_VALUE, "rung %d, target %d, plane %d is %dx%d, the rung began with %dx%d (one size per rung)", r, i, p, pairs[2 * p].w,
                                pairs[2 * p].h, d0.w, d0.h);
            }
        }
        rc = lanczos_one_source_size(pi + src_at, planes.data() + src_at, np, i);
        if (rc) return rc;
    }
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no planar Lanczos ladder kernels"));
    if (rc) return rc;
    // two tables per plane per rung (planes of one geometry share theirs)
    LanczosRef refs[2 * kLanczosPlanarMaxPlanes * CHV_LADDER_MAX_RUNGS];
    LanczosPlanarLadderJob job;
    memset(&job, 0, sizeof job);
    job.n_rungs = n_rungs; job.n_planes = np;
    for (int p = 0; p < np; p++) { job.src_w[p] = planes[src_at + p].w; job.src_h[p] = planes[src_at + p].h; }
    for (int r = 0; r < n_rungs; r++) {
        for (int p = 0; p < np; p++) {
            const DPlane &d = planes[r * np + p];
            LanczosRef *rp = &refs[2 * (r * kLanczosPlanarMaxPlanes + p)];
            rc = lanczos_table_pair(c, job.src_w[p], job.src_h[p], d.w, d.h, &rp[0], &rp[1], &job.rung[r].tab[p]);
            if (rc) return rc;
            job.rung[r].w[p] = d.w; job.rung[r].h[p] = d.h;
        }
    }
    return lanczos_send(c, planes.data(), per, n, lanczos_chunk(per), [&](DPlane *dev, int m) {
        job.batch = dev; job.n_pictures = m;
        int launches = 0;
        hipError_t e = launcher(job, c->stream, &launches);
        debug_counters().lanczos_planar_ladder_launches.fetch_add((unsigned long long)launches, std::memory_order_relaxed);
        return e != hipSuccess ? hip_fail(e, "lanczos planar ladder launch") : CHV_OK;
    });
}

// ---- chv_scale_lanczos_420 / chv_scale_lanczos_420_ladder: Lanczos-3 between NV12 and y420p ----
// Pictures per descriptor slot of a chunk: a picture's dnp target planes of every rung and its snp source planes, lanczos_chunk(n_rungs * dnp + snp).
static_assert(lanczos_chunk(3 * 2 + 3) == CHV_420_LADDER_CHUNK(3, 2, 3) && lanczos_chunk(8 * 3 + 2) == CHV_420_LADDER_CHUNK(8, 3, 2) &&
              lanczos_chunk(8 * 3 + 2) >= 1 && CHV_420_LADDER_CHUNK(4, 3, 3) == CHV_PLANAR_LADDER_CHUNK(4, 3) &&
              CHV_420_LADDER_CHUNK(5, 2, 2) == CHV_PLANAR_LADDER_CHUNK(5, 2),
              "a chunk is what fits one descriptor slot (include/chipvideo.h states the rule); same-format lists are chunked like chv_scale_lanczos_ladder");

// every plane of one 4:2:0 picture of either packing -> out[0 .. np); *np 0 and `err` for anything else.  A y420p picture's chroma planes
// must have one size: they are two images of one logical grid.
static int lanczos_420_planes(chv_context *c, const chv_image *img, int err, const char *what, int idx, DPlane *out, int *np) {
    *np = lanczos_planar_planes(img);
    if (!*np) return fail(err, "Lanczos 4:2:0 %s %d must be nv12 with 2 planes or y420p with 3", what, idx);
    for (int p = 0; p < *np; p++) {
        int rc = plane_to_device(img->planes[p], lanczos_planar_comps(img->format, p), c->device, &out[p], err, what, p);
        if (rc) return rc;
    }
    if (*np == 3 && (out[1].w != out[2].w || out[1].h != out[2].h))
        return fail(err, "Lanczos 4:2:0 %s %d: chroma planes of %dx%d and %dx%d (a y420p picture's planes 1 and 2 have one size)", what, idx, out[1].w, out[1].h,
                    out[2].w, out[2].h);
    return CHV_OK;
}

// Picture i's target planes, rung by rung -> pi[r * dnp + p]; every plane has the size of its place in the ladder's first picture (`first`)
static int lanczos_420_targets(chv_context *c, const chv_image *dsts, int n_rungs, int n, int i, int dnp, DPlane *pi, const DPlane *first) {
    int np = 0;
    for (int r = 0; r < n_rungs; r++) {
        int rc = lanczos_420_planes(c, &dsts[(size_t)r * n + i], CHV_ERR_BAD_TARGET, "target", r * n + i, pi + r * dnp, &np);
        if (rc) return rc;
        for (int p = 0; p < dnp; p++)
            if (pi[r * dnp + p].w != first[r * dnp + p].w || pi[r * dnp + p].h != first[r * dnp + p].h)
                return fail(CHV_ERR_INVALID_VALUE, "rung %d, target %d, plane %d is %dx%d, the rung began with %dx%d (one size per rung)", r, i, p,
                            pi[r * dnp + p].w, pi[r * dnp + p].h, first[r * dnp + p].w, first[r * dnp + p].h);
    }
    return CHV_OK;
}

// job->rung[r]: two tables per target plane — from the job's logical luma or chroma size to the plane's in the first picture — and that size
template <class Job>
static int lanczos_420_tables(chv_context *c, const DPlane *planes, int n_rungs, int dnp, LanczosRef *refs, Job *job) {
    for (int r = 0; r < n_rungs; r++) {
        for (int p = 0; p < dnp; p++) {
            const DPlane &d = planes[r * dnp + p];
            LanczosRef *rp = &refs[2 * (r * kLanczosPlanarMaxPlanes + p)];
            int rc = lanczos_table_pair(c, p ? job->chroma_w : job->luma_w, p ? job->chroma_h : job->luma_h, d.w, d.h, &rp[0], &rp[1], &job->rung[r].tab[p]);
            if (rc) return rc;
            job->rung[r].w[p] = d.w; job->rung[r].h[p] = d.h;
        }
    }
    return CHV_OK;
}

extern "C" int chv_scale_lanczos_420_ladder(chv_context *c, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    bool empty;
    int rc = lanczos_ladder_header(dsts, n_rungs, srcs, n, &empty);
    if (rc || empty) return rc;
    const Lanczos420Launcher launcher = g_lanczos_420_launcher.load(std::memory_order_acquire);
    const int dnp = lanczos_planar_planes(&dsts[0]), snp = lanczos_planar_planes(&srcs[0]);
    if (!dnp) return fail(CHV_ERR_BAD_TARGET, "Lanczos 4:2:0: target 0 must be nv12 with 2 planes or y420p with 3");
    if (!snp) return fail(CHV_ERR_BAD_INPUT, "Lanczos 4:2:0: source 0 must be nv12 with 2 planes or y420p with 3");
    rc = lanczos_ladder_formats(dsts, n_rungs, srcs, n);
    if (rc) return rc;
    // a picture's record: the dnp target planes of rung 0, of rung 1, ..., then the snp source planes
    const size_t per = (size_t)n_rungs * dnp + snp, src_at = (size_t)n_rungs * dnp;
    std::vector<DPlane> planes(per * n);
    DepScope deps;
    for (int i = 0; i < n; i++) {
        DPlane *pi = planes.data() + per * i;
        rc = lanczos_420_targets(c, dsts, n_rungs, n, i, dnp, pi, planes.data());
        if (rc) return rc;
        int np = 0;
        rc = lanczos_420_planes(c, &srcs[i], CHV_ERR_BAD_INPUT, "input", i, pi + src_at, &np);
        if (rc) return rc;
        rc = lanczos_one_source_size(pi + src_at, planes.data() + src_at, snp, i);
        if (rc) return rc;
    }
    // same-format lists are chv_scale_lanczos_ladder's: its launchers, its counter, its bytes
    if (dnp == snp) return chv_scale_lanczos_ladder(c, dsts, n_rungs, srcs, n);
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no 4:2:0 conversion Lanczos kernels"));
    if (rc) return rc;
    // two tables per logical plane per rung
    LanczosRef refs[2 * kLanczosPlanarMaxPlanes * CHV_LADDER_MAX_RUNGS];
    Lanczos420Job job;
    memset(&job, 0, sizeof job);
    job.n_rungs = n_rungs; job.dst_planes = dnp; job.src_planes = snp;
    job.luma_w = planes[src_at].w; job.luma_h = planes[src_at].h;
    job.chroma_w = planes[src_at + 1].w; job.chroma_h = planes[src_at + 1].h;
    rc = lanczos_420_tables(c, planes.data(), n_rungs, dnp, refs, &job);
    if (rc) return rc;
    return lanczos_send(c, planes.data(), per, n, lanczos_chunk(per), [&](DPlane *dev, int m) {
        job.batch = dev; job.n_pictures = m;
        int launches = 0;
        hipError_t e = launcher(job, c->stream, &launches);
        debug_counters().lanczos_420_ladder_launches.fetch_add((unsigned long long)launches, std::memory_order_relaxed);
        return e != hipSuccess ? hip_fail(e, "lanczos 4:2:0 ladder launch") : CHV_OK;
    });
}

extern "C" int chv_scale_lanczos_420(chv_context *c, const chv_image *dst, const chv_image *src) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    DPlane pl[kLanczosPlanarMaxPlanes];
    int dnp = 0, snp = 0;
    int rc = lanczos_420_planes(c, dst, CHV_ERR_BAD_TARGET, "target", 0, pl, &dnp);
    if (rc) return rc;
    rc = lanczos_420_planes(c, src, CHV_ERR_BAD_INPUT, "input", 0, pl, &snp);
    if (rc) return rc;
    // a same-format pair is chv_scale_lanczos's; a cross pair is the ladder of one rung and one picture
    return dnp == snp ? chv_scale_lanczos(c, dst, src) : chv_scale_lanczos_420_ladder(c, dst, 1, src, 1);
}

// ---- chv_scale_lanczos_to_420 / chv_scale_lanczos_to_420_ladder: the decoder's other five formats -> NV12 / y420p ----
static_assert(lanczos_chunk(4 * 2 + 1) == CHV_420_LADDER_CHUNK(4, 2, 1) && lanczos_chunk(8 * 3 + 3) >= 1, "a chunk is what fits one descriptor slot");

// planes of a source of one of the five formats, 0 for every other (format, structure); *kind: LanczosTo420Source
static int lanczos_to_420_kind(const chv_image *img, int *kind) {
    if (!img) return 0;
    switch (img->format) {
    case CHV_FMT_NV21: *kind = kTo420Nv21; return img->n_planes == 2 ? 2 : 0;
    case CHV_FMT_Y422P: case CHV_FMT_Y444P: *kind = kTo420Planar; return img->n_planes == 3 ? 3 : 0;
    case CHV_FMT_YUVS: *kind = kTo420Yuvs; return img->n_planes == 1 ? 1 : 0;
    case CHV_FMT_ZVUY: *kind = kTo420Zvuy; return img->n_planes == 1 ? 1 : 0;
    default: return 0;
    }
}

// every plane of one source of the five formats -> out[0 .. np), every check of plane_to_device on every plane; Cb and Cr must agree, a packed
// plane (2 bytes per pixel) must have an even width
static int lanczos_to_420_planes(chv_context *c, const chv_image *img, int np, int kind, int idx, DPlane *out) {
    int k2 = 0;
    if (lanczos_to_420_kind(img, &k2) != np || k2 != kind)
        return fail(CHV_ERR_BAD_INPUT, "Lanczos to 4:2:0: source %d must be nv21 (2 planes), y422p / y444p (3), yuvs / zvuy (1), nv12 or y420p", idx);
    for (int p = 0; p < np; p++) {
        const int comps = kind == kTo420Planar ? 1 : kind == kTo420Nv21 ? (p ? 2 : 1) : 2;
        int rc = plane_to_device(img->planes[p], comps, c->device, &out[p], CHV_ERR_BAD_INPUT, "input", p);
        if (rc) return rc;
    }
    if (np == 3 && (out[1].w != out[2].w || out[1].h != out[2].h))
        return fail(CHV_ERR_BAD_INPUT, "Lanczos to 4:2:0: source %d: chroma planes of %dx%d and %dx%d (Cb and Cr have one size)", idx, out[1].w, out[1].h, out[2].w, out[2].h);
    if (np == 1 && (out[0].w & 1))
        return fail(CHV_ERR_BAD_INPUT, "Lanczos to 4:2:0: source %d: a packed 4:2:2 picture of odd width %d", idx, out[0].w);
    return CHV_OK;
}

extern "C" int chv_scale_lanczos_to_420_ladder(chv_context *c, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    bool empty;
    int rc = lanczos_ladder_header(dsts, n_rungs, srcs, n, &empty);
    if (rc || empty) return rc;
    const LanczosTo420Launcher launcher = g_lanczos_to_420_launcher.load(std::memory_order_acquire);
    const int dnp = lanczos_planar_planes(&dsts[0]);
    if (!dnp) return fail(CHV_ERR_BAD_TARGET, "Lanczos to 4:2:0: target 0 must be nv12 with 2 planes or y420p with 3");
    // NV12 and y420p sources are chv_scale_lanczos_420_ladder's: its checks, its launchers, its counters, its bytes
    if (lanczos_planar_planes(&srcs[0])) return chv_scale_lanczos_420_ladder(c, dsts, n_rungs, srcs, n);
    int kind = 0;
    const int snp = lanczos_to_420_kind(&srcs[0], &kind);
    if (!snp) return fail(CHV_ERR_BAD_INPUT, "Lanczos to 4:2:0: source 0 must be nv21 (2 planes), y422p / y444p (3), yuvs / zvuy (1), nv12 or y420p");
    rc = lanczos_ladder_formats(dsts, n_rungs, srcs, n);
    if (rc) return rc;
    // a picture's record: the dnp target planes of rung 0, of rung 1, ..., then the snp source planes
    const size_t per = (size_t)n_rungs * dnp + snp, src_at = (size_t)n_rungs * dnp;
    std::vector<DPlane> planes(per * n);
    DepScope deps;
    for (int i = 0; i < n; i++) {
        DPlane *pi = planes.data() + per * i;
        rc = lanczos_420_targets(c, dsts, n_rungs, n, i, dnp, pi, planes.data());
        if (rc) return rc;
        rc = lanczos_to_420_planes(c, &srcs[i], snp, kind, i, pi + src_at);
        if (rc) return rc;
        rc = lanczos_one_source_size(pi + src_at, planes.data() + src_at, snp, i);
        if (rc) return rc;
    }
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no to-4:2:0 Lanczos kernels"));
    if (rc) return rc;
    // two tables per logical image per rung
    LanczosRef refs[2 * kLanczosPlanarMaxPlanes * CHV_LADDER_MAX_RUNGS];
    LanczosTo420Job job;
    memset(&job, 0, sizeof job);
    job.n_rungs = n_rungs; job.source = kind; job.dst_planes = dnp; job.src_planes = snp;
    job.luma_w = planes[src_at].w; job.luma_h = planes[src_at].h;
    // a packed plane's chroma images are width / 2 x height; every other source says their size itself
    job.chroma_w = snp == 1 ? planes[src_at].w / 2 : planes[src_at + 1].w;
    job.chroma_h = snp == 1 ? planes[src_at].h : planes[src_at + 1].h;
    rc = lanczos_420_tables(c, planes.data(), n_rungs, dnp, refs, &job);
    if (rc) return rc;
    return lanczos_send(c, planes.data(), per, n, lanczos_chunk(per), [&](DPlane *dev, int m) {
        job.batch = dev; job.n_pictures = m;
        int launches = 0;
        hipError_t e = launcher(job, c->stream, &launches);
        debug_counters().lanczos_to_420_launches.fetch_add((unsigned long long)launches, std::memory_order_relaxed);
        return e != hipSuccess ? hip_fail(e, "lanczos to 4:2:0 launch") : CHV_OK;
    });
}

extern "C" int chv_scale_lanczos_to_420(chv_context *c, const chv_image *dst, const chv_image *src) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (!lanczos_planar_planes(dst)) return fail(CHV_ERR_BAD_TARGET, "Lanczos to 4:2:0: the target must be nv12 with 2 planes or y420p with 3");
    if (!src) return fail(CHV_ERR_BAD_INPUT, "Lanczos to 4:2:0: null source");
    // an NV12 or y420p source is chv_scale_lanczos_420's; everything else is the ladder of one rung and one picture
    return lanczos_planar_planes(src) ? chv_scale_lanczos_420(c, dst, src) : chv_scale_lanczos_to_420_ladder(c, dst, 1, src, 1);
}

// ---- chv_scale_lanczos_hbd_to_420 / chv_scale_lanczos_hbd_to_420_ladder: P010, y420p10 -> NV12 / y420p ----
// planes of a source of one of the two 10-bit formats, 0 for every other (format, structure); *kind: LanczosHbdSource
static int lanczos_hbd_kind(const chv_image *img, int *kind) {
    if (!img) return 0;
    switch (img->format) {
    case CHV_FMT_P010: *kind = kHbdP010; return img->n_planes == 2 ? 2 : 0;
    case CHV_FMT_Y420P10: *kind = kHbdPlanar; return img->n_planes == 3 ? 3 : 0;
    default: return 0;
    }
}

// every plane of one 10-bit source -> out[0 .. np), every check of plane_to_device on every plane with components = bytes per texel (2; 4 for
// P010's CbCr); a 16-bit plane starts at an even address with an even pitch; Cb and Cr must agree
static int lanczos_hbd_planes(chv_context *c, const chv_image *img, int np, int kind, int idx, DPlane *out) {
    int k2 = 0;
    if (lanczos_hbd_kind(img, &k2) != np || k2 != kind)
        return fail(CHV_ERR_BAD_INPUT, "Lanczos 10-bit to 4:2:0: source %d must be p010 (2 planes) or y420p10 (3 planes)", idx);
    for (int p = 0; p < np; p++) {
        int rc = plane_to_device(img->planes[p], kind == kHbdP010 && p ? 4 : 2, c->device, &out[p], CHV_ERR_BAD_INPUT, "input", p, 2);
        if (rc) return rc;
    }
    if (np == 3 && (out[1].w != out[2].w || out[1].h != out[2].h))
        return fail(CHV_ERR_BAD_INPUT, "Lanczos 10-bit to 4:2:0: source %d: chroma planes of %dx%d and %dx%d (Cb and Cr have one size)", idx, out[1].w, out[1].h, out[2].w, out[2].h);
    return CHV_OK;
}

extern "C" int chv_scale_lanczos_hbd_to_420_ladder(chv_context *c, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    bool empty;
    int rc = lanczos_ladder_header(dsts, n_rungs, srcs, n, &empty);
    if (rc || empty) return rc;
    const LanczosHbdLauncher launcher = g_lanczos_hbd_launcher.load(std::memory_order_acquire);
    const int dnp = lanczos_planar_planes(&dsts[0]);
    if (!dnp) return fail(CHV_ERR_BAD_TARGET, "Lanczos 10-bit to 4:2:0: target 0 must be nv12 with 2 planes or y420p with 3");
    int kind = 0;
    const int snp = lanczos_hbd_kind(&srcs[0], &kind);
    if (!snp) return fail(CHV_ERR_BAD_INPUT, "Lanczos 10-bit to 4:2:0: source 0 must be p010 (2 planes) or y420p10 (3 planes)");
    rc = lanczos_ladder_formats(dsts, n_rungs, srcs, n);
    if (rc) return rc;
    // a picture's record: the dnp target planes of rung 0, of rung 1, ..., then the snp source planes
    const size_t per = (size_t)n_rungs * dnp + snp, src_at = (size_t)n_rungs * dnp;
    std::vector<DPlane> planes(per * n);
    DepScope deps;
    for (int i = 0; i < n; i++) {
        DPlane *pi = planes.data() + per * i;
        rc = lanczos_420_targets(c, dsts, n_rungs, n, i, dnp, pi, planes.data());
        if (rc) return rc;
        rc = lanczos_hbd_planes(c, &srcs[i], snp, kind, i, pi + src_at);
        if (rc) return rc;
        rc = lanczos_one_source_size(pi + src_at, planes.data() + src_at, snp, i);
        if (rc) return rc;
    }
    const DPlane *s0 = planes.data() + src_at;
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no 10-bit Lanczos kernels"));
    if (rc) return rc;
    // two tables per logical image per rung
    LanczosRef refs[2 * kLanczosPlanarMaxPlanes * CHV_LADDER_MAX_RUNGS];
    LanczosHbdJob job;
    memset(&job, 0, sizeof job);
    job.n_rungs = n_rungs; job.source = kind; job.dst_planes = dnp; job.src_planes = snp;
    job.luma_w = s0[0].w; job.luma_h = s0[0].h;
    job.chroma_w = s0[1].w; job.chroma_h = s0[1].h;
    rc = lanczos_420_tables(c, planes.data(), n_rungs, dnp, refs, &job);
    if (rc) return rc;
    return lanczos_send(c, planes.data(), per, n, lanczos_chunk(per), [&](DPlane *dev, int m) {
        job.batch = dev; job.n_pictures = m;
        int launches = 0;
        hipError_t e = launcher(job, c->stream, &launches);
        debug_counters().lanczos_hbd_launches.fetch_add((unsigned long long)launches, std::memory_order_relaxed);
        return e != hipSuccess ? hip_fail(e, "lanczos 10-bit launch") : CHV_OK;
    });
}

extern "C" int chv_scale_lanczos_hbd_to_420(chv_context *c, const chv_image *dst, const chv_image *src) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (!lanczos_planar_planes(dst)) return fail(CHV_ERR_BAD_TARGET, "Lanczos 10-bit to 4:2:0: the target must be nv12 with 2 planes or y420p with 3");
    if (!src) return fail(CHV_ERR_BAD_INPUT, "Lanczos 10-bit to 4:2:0: null source");
    // the ladder of one rung and one picture
    return chv_scale_lanczos_hbd_to_420_ladder(c, dst, 1, src, 1);
}

// ---- chv_scale_lanczos_from_yuv: an NV12 or y420p picture -> one BGRA / RGBA plane ----
// Pictures per descriptor slot of a batch chunk: a picture's target plane and its np source planes, lanczos_chunk(1 + np) — the counts of
// chv_scale_lanczos_to_yuv_batch, whose pictures have as many plane records.
static_assert(lanczos_chunk(1 + 2) == 83 && lanczos_chunk(1 + 3) == 62, "include/chipvideo.h states the counts");

// DESIGN.md section 4.2's table (the device's copy is kCsc, pixel_math.hip.h): yoff, cy, crv, cgu, cgv, cbu
static const int32_t kY2RHost[4][6] = {
    { 16, 76309, 104597, 25675, 53279, 132201 },  // BT.601 limited
    { 16, 76309, 117489, 13975, 34925, 138438 },  // BT.709 limited
    { 0, 65536, 91881, 22553, 46802, 116130 },    // BT.601 full
    { 0, 65536, 103206, 12276, 30679, 121609 },   // BT.709 full
};

// (dst, src) of one picture -> its target plane at out[0], its np source planes at out[1 .. np]; every check of plane_to_device
static int lanczos_from_yuv_planes(chv_context *c, const chv_image *dst, const chv_image *src, int idx, DPlane *out, int *np) {
    if (!dst || dst->n_planes != 1 || (dst->format != CHV_FMT_BGRA && dst->format != CHV_FMT_RGBA))
        return fail(CHV_ERR_BAD_TARGET, "Lanczos from YUV: target %d must be one 4-component plane of format BGRA or RGBA", idx);
    int rc = plane_to_device(dst->planes[0], 4, c->device, &out[0], CHV_ERR_BAD_TARGET, "target", 0);
    if (rc) return rc;
    *np = lanczos_planar_planes(src);
    if (!*np) return fail(CHV_ERR_BAD_INPUT, "Lanczos from YUV: source %d must be nv12 with 2 planes or y420p with 3", idx);
    for (int p = 0; p < *np; p++) {
        rc = plane_to_device(src->planes[p], lanczos_planar_comps(src->format, p), c->device, &out[1 + p], CHV_ERR_BAD_INPUT, "input", p);
        if (rc) return rc;
        if (p && (out[1 + p].w != std::max(1, out[1].w / 2) || out[1 + p].h != std::max(1, out[1].h / 2)))
            return fail(CHV_ERR_BAD_INPUT, "Lanczos from YUV: source %d, plane %d is %dx%d, a %dx%d picture's chroma is %dx%d", idx, p, out[1 + p].w,
                        out[1 + p].h, out[1].w, out[1].h, std::max(1, out[1].w / 2), std::max(1, out[1].h / 2));
    }
    return CHV_OK;
}

// section 4.2's row for `opts` (NULL: BT.601 limited) into a LanczosFromYuvJob or a LanczosFromYuvLadderJob
template <class Job>
static void lanczos_from_yuv_matrix(const chv_kernel_opts *opts, Job *job) {
    const int32_t *k = kY2RHost[(opts ? opts->colorspace : CHV_CSC_BT601_LIMITED) & 3];
    job->yoff = k[0]; job->cy = k[1]; job->crv = k[2]; job->cgu = k[3]; job->cgv = k[4]; job->cbu = k[5];
}

// the four tables of one geometry (held in refs until the launch is enqueued) and everything else of the job but the batch
static int lanczos_from_yuv_job(chv_context *c, const DPlane *planes, int np, int dst_format, const chv_kernel_opts *opts, LanczosRef *refs,
                                LanczosFromYuvJob *job) {
    memset(job, 0, sizeof *job);
    for (int p = 0; p < 2; p++) {
        const DPlane &s = planes[1 + p];
        int rc = lanczos_table_pair(c, s.w, s.h, planes[0].w, planes[0].h, &refs[2 * p], &refs[2 * p + 1], p ? &job->chroma : &job->luma);
        if (rc) return rc;
    }
    job->dst = planes[0];
    for (int p = 0; p < np; p++) job->src[p] = planes[1 + p];
    job->src_planes = np;
    job->rgba = dst_format == CHV_FMT_RGBA;
    lanczos_from_yuv_matrix(opts, job);
    return CHV_OK;
}

extern "C" int chv_scale_lanczos_from_yuv(chv_context *c, const chv_image *dst, const chv_image *src, const chv_kernel_opts *opts) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    const LanczosFromYuvLauncher launcher = g_lanczos_from_yuv_launcher.load(std::memory_order_acquire);
    DPlane planes[1 + kLanczosPlanarMaxPlanes];
    DepScope deps;
    int np = 0;
    int rc = lanczos_from_yuv_planes(c, dst, src, 0, planes, &np);
    if (rc) return rc;
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no Lanczos from YUV kernels"));
    if (rc) return rc;
    LanczosRef refs[4];      // held until the launch is enqueued (see LanczosTable)
    LanczosFromYuvJob job;
    rc = lanczos_from_yuv_job(c, planes, np, dst->format, opts, refs, &job);
    if (rc) return rc;
    job.batch = nullptr; job.n_pictures = 1;
    (void)hipGetLastError();
    hipError_t e = launcher(job, c->stream);
    if (e != hipSuccess) return hip_fail(e, "lanczos from YUV launch");
    debug_counters().lanczos_from_yuv_launches.fetch_add(1, std::memory_order_relaxed);
    return CHV_OK;
}

extern "C" int chv_scale_lanczos_from_yuv_batch(chv_context *c, const chv_image *dsts, const chv_image *srcs, int n, const chv_kernel_opts *opts) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (n == 0) return CHV_OK;
    if (n < 0 || !dsts || !srcs) return fail(CHV_ERR_INVALID_VALUE, "bad batch");
    const LanczosFromYuvLauncher launcher = g_lanczos_from_yuv_launcher.load(std::memory_order_acquire);
    // (one target format and one source format per batch: the list's mistake, not the image's — before anything else is looked at)
    for (int i = 1; i < n; i++) {
        if (dsts[i].format != dsts[0].format)
            return fail(CHV_ERR_INVALID_VALUE, "target %d has format %d, the batch began with %d (one target format per batch)", i, dsts[i].format, dsts[0].format);
        if (srcs[i].format != srcs[0].format)
            return fail(CHV_ERR_INVALID_VALUE, "source %d has format %d, the batch began with %d (one source format per batch)", i, srcs[i].format, srcs[0].format);
    }
    DPlane first[1 + kLanczosPlanarMaxPlanes];
    DepScope deps;
    int np = 0;
    int rc = lanczos_from_yuv_planes(c, &dsts[0], &srcs[0], 0, first, &np);
    if (rc) return rc;
    const size_t per = (size_t)np + 1;
    std::vector<DPlane> planes(per * n);
    std::copy(first, first + per, planes.begin());
    for (int i = 1; i < n; i++) {
        DPlane pi[1 + kLanczosPlanarMaxPlanes];
        int npi = 0;
        rc = lanczos_from_yuv_planes(c, &dsts[i], &srcs[i], i, pi, &npi);
        if (rc) return rc;
        if (npi != np) return fail(CHV_ERR_INVALID_VALUE, "source %d has %d planes, the batch began with %d (one source format per batch)", i, npi, np);
        if (pi[0].w != first[0].w || pi[0].h != first[0].h || pi[1].w != first[1].w || pi[1].h != first[1].h)
            return fail(CHV_ERR_INVALID_VALUE, "pair %d: %dx%d -> %dx%d, the batch is %dx%d -> %dx%d (one geometry per batch)", i,
                        pi[1].w, pi[1].h, pi[0].w, pi[0].h, first[1].w, first[1].h, first[0].w, first[0].h);
        std::copy(pi, pi + per, planes.begin() + per * i);
    }
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no Lanczos from YUV kernels"));
    if (rc) return rc;
    LanczosRef refs[4];
    LanczosFromYuvJob job;
    rc = lanczos_from_yuv_job(c, planes.data(), np, dsts[0].format, opts, refs, &job);
    if (rc) return rc;
    return lanczos_send(c, planes.data(), per, n, lanczos_chunk(per), [&](DPlane *dev, int m) {
        job.batch = dev; job.n_pictures = m;
        hipError_t e = launcher(job, c->stream);
        if (e != hipSuccess) return hip_fail(e, "lanczos from YUV launch");
        debug_counters().lanczos_from_yuv_launches.fetch_add(1, std::memory_order_relaxed);      // (only launches that were made)
        return (int)CHV_OK;
    });
}

// ---- chv_scale_lanczos_from_yuv_ladder: every BGRA / RGBA rendition of every decoded picture in one launch per route ----
// Pictures per descriptor slot: a picture's n_rungs target planes and its snp source planes, lanczos_chunk(n_rungs + snp).
// include/chipvideo.h states the rule as CHV_FROM_YUV_LADDER_CHUNK; with one rung it gives the batch's counts.
static_assert(CHV_FROM_YUV_LADDER_CHUNK(1, 2) == lanczos_chunk(1 + 2) && CHV_FROM_YUV_LADDER_CHUNK(1, 3) == lanczos_chunk(1 + 3) &&
              CHV_FROM_YUV_LADDER_CHUNK(1, 2) == 83 && CHV_FROM_YUV_LADDER_CHUNK(1, 3) == 62 &&
              lanczos_chunk(8 + 2) == CHV_FROM_YUV_LADDER_CHUNK(8, 2) && lanczos_chunk(8 + 3) == CHV_FROM_YUV_LADDER_CHUNK(8, 3) &&
              lanczos_chunk(CHV_LADDER_MAX_RUNGS + 3) >= 1,
              "a chunk is what fits one descriptor slot (include/chipvideo.h states the rule); one rung is chunked like chv_scale_lanczos_from_yuv_batch");

extern "C" int chv_scale_lanczos_from_yuv_ladder(chv_context *c, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n, const chv_kernel_opts *opts) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    bool empty;
    int rc = lanczos_ladder_header(dsts, n_rungs, srcs, n, &empty);
    if (rc || empty) return rc;
    const LanczosFromYuvLadderLauncher launcher = g_lanczos_from_yuv_ladder_launcher.load(std::memory_order_acquire);
    rc = lanczos_ladder_formats(dsts, n_rungs, srcs, n);
    if (rc) return rc;
    // a picture's record: the target plane of rung 0, of rung 1, ..., then the snp source planes
    const int snp0 = lanczos_planar_planes(&srcs[0]);
    const int snp = snp0 ? snp0 : 2;                   // (a source that is neither packing is refused below, by its own status)
    const size_t per = (size_t)n_rungs + snp, src_at = (size_t)n_rungs;
    std::vector<DPlane> planes(per * n);
    DepScope deps;
    for (int i = 0; i < n; i++) {
        DPlane *pi = planes.data() + per * i;
        for (int r = 0; r < n_rungs; r++) {
            DPlane one[1 + kLanczosPlanarMaxPlanes];
            int np = 0;
            rc = lanczos_from_yuv_planes(c, &dsts[(size_t)r * n + i], &srcs[i], r * n + i, one, &np);
            if (rc) return rc;
            if (np != snp) return fail(CHV_ERR_INVALID_VALUE, "source %d has %d planes, the ladder began with %d (one source format per ladder)", i, np, snp);
            pi[r] = one[0];
            if (r == 0) std::copy(one + 1, one + 1 + snp, pi + src_at);
            if (pi[r].w != planes[r].w || pi[r].h != planes[r].h)
                return fail(CHV_ERR_INVALID_VALUE, "rung %d, target %d is %dx%d, the rung began with %dx%d (one size per rung)", r, i, pi[r].w, pi[r].h,
                            planes[r].w, planes[r].h);
        }
        if (pi[src_at].w != planes[src_at].w || pi[src_at].h != planes[src_at].h)
            return fail(CHV_ERR_INVALID_VALUE, "source %d is %dx%d, the ladder began with %dx%d (one source size per ladder)", i, pi[src_at].w, pi[src_at].h,
                        planes[src_at].w, planes[src_at].h);
    }
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no Lanczos from YUV ladder kernels"));
    if (rc) return rc;
    // four tables per rung
    LanczosRef refs[4 * CHV_LADDER_MAX_RUNGS];
    LanczosFromYuvLadderJob job;
    memset(&job, 0, sizeof job);
    job.n_rungs = n_rungs; job.src_planes = snp;
    job.rgba = dsts[0].format == CHV_FMT_RGBA;
    job.luma_w = planes[src_at].w; job.luma_h = planes[src_at].h;
    job.chroma_w = planes[src_at + 1].w; job.chroma_h = planes[src_at + 1].h;
    lanczos_from_yuv_matrix(opts, &job);
    for (int r = 0; r < n_rungs; r++) {
        LanczosFromYuvLadderRung &R = job.rung[r];
        R.w = planes[r].w; R.h = planes[r].h;
        for (int p = 0; p < 2; p++) {
            LanczosRef *rp = &refs[4 * r + 2 * p];
            rc = lanczos_table_pair(c, p ? job.chroma_w : job.luma_w, p ? job.chroma_h : job.luma_h, R.w, R.h, &rp[0], &rp[1], p ? &R.chroma : &R.luma);
            if (rc) return rc;
        }
    }
    return lanczos_send(c, planes.data(), per, n, lanczos_chunk(per), [&](DPlane *dev, int m) {
        job.batch = dev; job.n_pictures = m;
        int launches = 0;
        hipError_t e = launcher(job, c->stream, &launches);
        debug_counters().lanczos_from_yuv_ladder_launches.fetch_add((unsigned long long)launches, std::memory_order_relaxed);
        return e != hipSuccess ? hip_fail(e, "lanczos from YUV ladder launch") : CHV_OK;
    });
}

// ---- chv_scale_lanczos_rgb_ladder: every rendition of every 4-component plane in one launch per route ----
// Pictures per descriptor slot: a picture's n_rungs target planes and its source plane, lanczos_chunk(n_rungs + 1).
// include/chipvideo.h states the rule as CHV_RGB_LADDER_CHUNK.
static_assert(CHV_RGB_LADDER_CHUNK(1) == 124 && CHV_RGB_LADDER_CHUNK(8) == 27 &&
              lanczos_chunk(1 + 1) == CHV_RGB_LADDER_CHUNK(1) && lanczos_chunk(4 + 1) == CHV_RGB_LADDER_CHUNK(4) &&
              lanczos_chunk(CHV_LADDER_MAX_RUNGS + 1) == CHV_RGB_LADDER_CHUNK(CHV_LADDER_MAX_RUNGS) && lanczos_chunk(CHV_LADDER_MAX_RUNGS + 1) >= 1,
              "a chunk is what fits one descriptor slot (include/chipvideo.h states the rule)");

extern "C" int chv_scale_lanczos_rgb_ladder(chv_context *c, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    bool empty;
    int rc = lanczos_ladder_header(dsts, n_rungs, srcs, n, &empty);
    if (rc || empty) return rc;
    const LanczosRgbLadderLauncher launcher = g_lanczos_rgb_ladder_launcher.load(std::memory_order_acquire);
    // a picture's record: the target plane of rung 0, of rung 1, ..., then the source plane
    const size_t per = (size_t)n_rungs + 1, src_at = (size_t)n_rungs;
    std::vector<DPlane> planes(per * n);
    DepScope deps;
    for (int i = 0; i < n; i++) {
        DPlane *pi = planes.data() + per * i;
        for (int r = 0; r < n_rungs; r++) {
            const chv_image &d = dsts[(size_t)r * n + i];
            if (d.n_planes != 1) return fail(CHV_ERR_BAD_TARGET, "Lanczos RGB ladder: rung %d, target %d must be one 4-component plane", r, i);
            rc = plane_to_device(d.planes[0], 4, c->device, &pi[r], CHV_ERR_BAD_TARGET, "target", r * n + i);
            if (rc) return rc;
            if (pi[r].w != planes[r].w || pi[r].h != planes[r].h)
                return fail(CHV_ERR_INVALID_VALUE, "rung %d, target %d is %dx%d, the rung began with %dx%d (one size per rung)", r, i, pi[r].w, pi[r].h,
                            planes[r].w, planes[r].h);
        }
        if (srcs[i].n_planes != 1) return fail(CHV_ERR_BAD_INPUT, "Lanczos RGB ladder: source %d must be one 4-component plane", i);
        rc = plane_to_device(srcs[i].planes[0], 4, c->device, &pi[src_at], CHV_ERR_BAD_INPUT, "input", i);
        if (rc) return rc;
        if (pi[src_at].w != planes[src_at].w || pi[src_at].h != planes[src_at].h)
            return fail(CHV_ERR_INVALID_VALUE, "source %d is %dx%d, the ladder began with %dx%d (one source size per ladder)", i, pi[src_at].w, pi[src_at].h,
                        planes[src_at].w, planes[src_at].h);
    }
    rc = lanczos_begin(c, deps, launcher ? CHV_OK : fail(CHV_ERR_NOT_IMPLEMENTED, "this build has no Lanczos RGB ladder kernels"));
    if (rc) return rc;
    // two tables per rung
    LanczosRef refs[2 * CHV_LADDER_MAX_RUNGS];
    LanczosRgbLadderJob job;
    memset(&job, 0, sizeof job);
    job.n_rungs = n_rungs;
    job.src_w = planes[src_at].w; job.src_h = planes[src_at].h;
    for (int r = 0; r < n_rungs; r++) {
        LanczosRgbLadderRung &R = job.rung[r];
        R.w = planes[r].w; R.h = planes[r].h;
        rc = lanczos_table_pair(c, job.src_w, job.src_h, R.w, R.h, &refs[2 * r], &refs[2 * r + 1], &R.tab);
        if (rc) return rc;
    }
    return lanczos_send(c, planes.data(), per, n, lanczos_chunk(per), [&](DPlane *dev, int m) {
        job.batch = dev; job.n_pictures = m;
        int launches = 0;
        hipError_t e = launcher(job, c->stream, &launches);
        debug_counters().lanczos_rgb_ladder_launches.fetch_add((unsigned long long)launches, std::memory_order_relaxed);
        return e != hipSuccess ? hip_fail(e, "lanczos RGB ladder launch") : CHV_OK;
    });
}

// ---------------------------------------------------------------------------
// events
// ---------------------------------------------------------------------------
extern "C" int chv_event_create(chv_context *c, chv_event **out) {
    if (!out) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    *out = nullptr;
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    HIP_TRY(hipSetDevice(c->device));
    hipEvent_t ev;
    HIP_TRY(hipEventCreate(&ev));
    chv_event *e = new chv_event;
    e->ev = ev; e->device = c->device;
    *out = e;
    return CHV_OK;
}
extern "C" int chv_event_record(chv_context *c, chv_event *ev) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (!ev || !ev->ev) return fail(CHV_ERR_INVALID_VALUE, "bad event");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(ev->ev, c->stream));
    return CHV_OK;
}
extern "C" int chv_event_wait(chv_context *c, chv_event *ev) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    if (!ev || !ev->ev) return fail(CHV_ERR_INVALID_VALUE, "bad event");
    if (ev->device != c->device) return fail(CHV_ERR_INVALID_VALUE, "event belongs to device %d", ev->device);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamWaitEvent(c->stream, ev->ev, 0));
    return CHV_OK;
}
extern "C" int chv_event_synchronize(chv_event *ev) {
    if (!ev || !ev->ev) return fail(CHV_ERR_INVALID_VALUE, "bad event");
    HIP_TRY(hipSetDevice(ev->device));
    HIP_TRY(hipEventSynchronize(ev->ev));
    return CHV_OK;
}
extern "C" int chv_event_elapsed_ms(chv_event *a, chv_event *b, float *ms) {
    if (!a || !b || !ms) return fail(CHV_ERR_INVALID_VALUE, "null argument");
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipEventElapsedTime(ms, a->ev, b->ev));
    return CHV_OK;
}
extern "C" int chv_event_destroy(chv_event *ev) {
    if (!ev) return fail(CHV_ERR_INVALID_VALUE, "null event");
    (void)hipSetDevice(ev->device);
    if (ev->ev) (void)hipEventDestroy(ev->ev);
    delete ev;
    return CHV_OK;
}
extern "C" int chv_device_synchronize(chv_context *c) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    FLUSH_PENDING(c);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    return CHV_OK;
}

// ---------------------------------------------------------------------------
// device self-test of the primitive conversions; not part of chipvideo.h
// (bound by tests/test_gpu_primitives.py only)
// ---------------------------------------------------------------------------
extern "C" int chv_selftest_primitives(chv_context *c, float *unorm_out /*256*/, const float *in_f,
                                       uint8_t *codes_out, const float *num, const float *den,
                                       float *quot_out, int n) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (n < 0 || !unorm_out) return fail(CHV_ERR_INVALID_VALUE, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    float *d_f = nullptr, *d_in = nullptr, *d_num = nullptr, *d_den = nullptr, *d_q = nullptr;
    uint8_t *d_c = nullptr;
    size_t m = n > 0 ? (size_t)n : 1;
    HIP_TRY(hipMalloc((void **)&d_f, 256 * sizeof(float)));
    HIP_TRY(hipMalloc((void **)&d_in, m * sizeof(float)));
    HIP_TRY(hipMalloc((void **)&d_num, m * sizeof(float)));
    HIP_TRY(hipMalloc((void **)&d_den, m * sizeof(float)));
    HIP_TRY(hipMalloc((void **)&d_q, m * sizeof(float)));
    HIP_TRY(hipMalloc((void **)&d_c, m));
    if (n > 0) {
        HIP_TRY(hipMemcpy(d_in, in_f, n * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_num, num, n * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_den, den, n * sizeof(float), hipMemcpyHostToDevice));
    }
    hipError_t e = launch_selftest(d_f, d_in, d_c, d_num, d_den, d_q, n, c->stream);
    if (e != hipSuccess) return hip_fail(e, "selftest launch");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(unorm_out, d_f, 256 * sizeof(float), hipMemcpyDeviceToHost));
    if (n > 0) {
        HIP_TRY(hipMemcpy(codes_out, d_c, n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(quot_out, d_q, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    (void)hipFree(d_f); (void)hipFree(d_in); (void)hipFree(d_num); (void)hipFree(d_den); (void)hipFree(d_q); (void)hipFree(d_c);
    return CHV_OK;
}

extern "C" int chv_selftest_pack(chv_context *c, const int *b, const int *g, const int *r, uint32_t *out /*2n*/, int n) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (n <= 0) return fail(CHV_ERR_INVALID_VALUE, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    int *d_b = nullptr, *d_g = nullptr, *d_r = nullptr; uint32_t *d_o = nullptr;
    HIP_TRY(hipMalloc((void **)&d_b, n * 4)); HIP_TRY(hipMalloc((void **)&d_g, n * 4)); HIP_TRY(hipMalloc((void **)&d_r, n * 4));
    HIP_TRY(hipMalloc((void **)&d_o, n * 8));
    HIP_TRY(hipMemcpy(d_b, b, n * 4, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(d_g, g, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_r, r, n * 4, hipMemcpyHostToDevice));
    hipError_t e = launch_selftest_pack(d_b, d_g, d_r, d_o, n, c->stream);
    if (e != hipSuccess) return hip_fail(e, "selftest launch");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, d_o, n * 8, hipMemcpyDeviceToHost));
    (void)hipFree(d_b); (void)hipFree(d_g); (void)hipFree(d_r); (void)hipFree(d_o);
    return CHV_OK;
}

// Exhaustive device self-test of the integer BT.601 / 709 matrices (tests/test_gpu_matrices.py): direction 0 YUV -> RGB (out[Y << 16 | U << 8 | V]
// = the BGRA word), 1 RGB -> YUV (out[R << 16 | G << 8 | B] = Y | U << 8 | V << 16), all 2^24 triples of colourspace `csc`; *mismatches = triples
// on which the forms of the YUV -> RGB matrix the kernels use disagree among themselves (direction 0).
extern "C" int chv_selftest_matrices(chv_context *c, int direction, int csc, uint32_t *out /* 1 << 24 */, uint32_t *mismatches) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (!out || !mismatches || direction < 0 || direction > 1 || csc < 0 || csc > 3) return fail(CHV_ERR_INVALID_VALUE, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    uint32_t *d_o = nullptr, *d_m = nullptr;
    const size_t bytes = sizeof(uint32_t) << 24;
    HIP_TRY(hipMalloc((void **)&d_o, bytes));
    hipError_t e = hipMalloc((void **)&d_m, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(d_m, 0, sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = launch_selftest_matrices(direction, csc, d_o, d_m, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_o, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(mismatches, d_m, sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_o); if (d_m) (void)hipFree(d_m);
    return e == hipSuccess ? CHV_OK : hip_fail(e, "selftest matrices");
}

extern "C" int chv_selftest_pack_codes(chv_context *c, const float *in /*4n*/, uint32_t *out /*2n*/, int n) {
    if (!ctx_ok(c)) return fail(CHV_ERR_INVALID_CONTEXT, "bad context");
    if (n <= 0 || !in || !out) return fail(CHV_ERR_INVALID_VALUE, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    float *d_in = nullptr; uint32_t *d_o = nullptr;
    HIP_TRY(hipMalloc((void **)&d_in, (size_t)n * 16));
    hipError_t e = hipMalloc((void **)&d_o, (size_t)n * 8);
    if (e == hipSuccess) e = hipMemcpy(d_in, in, (size_t)n * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_selftest_pack_codes(d_in, d_o, n, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_o, (size_t)n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d_in); if (d_o) (void)hipFree(d_o);
    return e == hipSuccess ? CHV_OK : hip_fail(e, "selftest pack_codes");
}
