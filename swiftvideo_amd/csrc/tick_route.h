// tick_route.h — which kernel runs a compositing tick: the route rules, the one plan they need (plan_wave_layers) and the
// compile-time numbers they read, for the host runtime (chipvideo.cpp, geom_store.cpp), the launchers in the kernel units and the CPU test
// (tests/cpp/test_tick_route.cpp).  Definitions: tick_route.cpp.  Plain C++: nothing here or there needs a GPU compiler.
//
// The numbers below are the kernels' own: each has its one definition here, the device side includes this header, and where a kernel's layout
// produces the number (a table's size, a ring's bytes) a static_assert next to that layout ties the two.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "device_types.h"

// build-variant defaults (tools/build_variant.sh -D...: one flag reaches the rules and the kernels)
#ifndef CHV_TW
#define CHV_TW 128
#endif
#ifndef CHV_KT
#define CHV_KT 4
#endif
// Waves per block of the strip kernels.  The waves of a block share nothing but the launch (every wave has its own LDS region and there is no
// block barrier on the data path), so the block size only sets the granularity at which LDS is handed out: one wave per block (1, 2 and 4
// measured the same where LDS is not the limit).
#ifndef CHV_WAVE_WAVES
#define CHV_WAVE_WAVES 1
#endif
// 1: rectangles taller than two rows per strip row are staged as the rows' own tap-row pairs (WGeom::pair, wave_common.hip.h)
#ifndef CHV_WAVE_PAIR
#define CHV_WAVE_PAIR 1
#endif
// rows of slack in a staged rectangle beyond ceil(strip rows x vertical ratio): tap row 1, and the ratio's rounding on both sides
#ifndef CHV_P0ROWS_SLACK
#define CHV_P0ROWS_SLACK 3
#endif

namespace chv {

// ---- the kernels' numbers ----------------------------------------------------------------------------------------------------------------
constexpr int NTHREADS = 256;            // threads per block of the tiled kernel
constexpr int LDS_BUDGET = 64 * 1024;    // LDS a block of the tiled / strip kernels may ask for
constexpr int WTW = 64;                  // strip width of the strip kernels: one lane per column
constexpr int WAVES = CHV_WAVE_WAVES;
// the tiled kernel (kernels_fast.hip.cpp)
constexpr int TW = CHV_TW;               // tile width (output pixels), a multiple of 64
constexpr int KT = CHV_KT;               // tiles per block: a vertical strip of KT tiles shares its column tables
// Tile height (output rows) is a kernel template parameter THV: 32 rows for launches that fill the chip anyway (more pixels
// per barrier interval: -6 % on cfg2), 16 rows for small launches such as a single mixer tick (twice the blocks: 9.6 instead
// of 12.3 us for one 720p tick).  RPT = THV / TYT rows per thread.
constexpr int TH_SMALL = 16, TH_LARGE = 32;
// sizeof(TileTablesT<th>): five column arrays, five row arrays, a summary per column wave and per tile
constexpr size_t tile_tables_bytes(int th) { return (size_t)4 * (5 * TW + 5 * KT * th) + (size_t)32 * (TW / 64 + KT); }
// tick_bgra_stream (kernels_stream_body.hip.inc): bytes per ring row of a planar chroma plane
constexpr int ST_CPP = 96;
// tick_yuv_stream (kernels_stream_yuv.hip.cpp)
constexpr int YS_MAXL = 4;               // layers per tick
constexpr int YS_TAB_BYTES = 416;        // a layer's row tables (YS_TAB_DW dwords)
constexpr int YS_RING_Y_BYTES = 3072, YS_RING_C2_BYTES = 1536, YS_RING_CP_BYTES = 2304;      // a layer's luma / NV12 chroma / planar chroma ring (RingY, RingC2, RingCP)
constexpr int YS_RING_RGB_PITCH = 320;   // bytes per row of an RGB layer's ring (RingRGB)
// kinds a launch contains (template parameter KINDS; the instantiation holds no code for the others)
enum { YK_NV12 = 1, YK_PLANAR = 2, YK_RGB = 4, YK_RGBINT = 8 };
// RGB texels, rows of 320 B: four batches of three rows in RGB-only launches (the encoder side), of two rows where video layers share the LDS
// (a mixer's overlays: the ring follows every row, and with two batches of three a row's request was two rows ahead of its taps — 600 ns of
// waiting per overlay row)
constexpr int ys_rgb_b(int kinds) { return (kinds & (YK_NV12 | YK_PLANAR)) ? 2 : 3; }
constexpr int ys_layer_bytes_c(bool rgb, bool planar, int rgb_b) {
    return rgb ? rgb_b * 4 * YS_RING_RGB_PITCH : YS_RING_Y_BYTES + (planar ? YS_RING_CP_BYTES : YS_RING_C2_BYTES);
}
// a colour matrix whose red and blue offsets fold into the conversion biases (pixel_math.hip.h: all but BT.601 full range)
constexpr bool csc_absorbable(int csc) { return (csc & 3) != 2; }

// ---- routes --------------------------------------------------------------------------------------------------------------------------------
// The ids travel as plain int (chipvideo.cpp keeps -1 / -2 for "general" / "none"); the names live in a namespace of their own so that a unit
// which includes this header for the declarations alone gets no enumerators (`using namespace chv::fast_path_ids;` where they are wanted).
namespace fast_path_ids {
enum FastPath : int { FP_NONE = -1, FP_NV12_BGRA_TILED = 0, FP_Y420P_BGRA_TILED = 1, FP_WAVE_LAYERS = 2, FP_WAVE_NV12 = 3, FP_WAVE_Y420P = 4, FP_STREAM = 5, FP_CLEAR_BGRA = 6, FP_STREAM_NV12 = 7, FP_STREAM_Y420P = 8, FP_COUNT };
}
const char *fast_path_name(int path);
bool fast_path_is_wave(int path);                // the strip kernels (they take per-layer geometry tables: geom_cache.h)
bool fast_path_by_value(int path);
int fast_path_stream_bgra();
// transient: one tick, launched once (its descriptors can travel as kernel arguments)
int select_fast_path(int target_format, const DTick *ticks, const DLayer *layers, int n_ticks, bool transient = false);
int select_single_purpose(const DTick *ticks, const DLayer *layers, int n_ticks);
int split_stream_prefix(const DTick *ticks, const DLayer *layers, int n_ticks);
int select_tail_path(int target_format, const DTick *ticks, const DLayer *layers, int n_ticks);      // the path of a split batch's second launch

bool finite16(const float *m);

// ---- the tiled kernel (kernels_fast.hip.cpp) ---------------------------------------------------------------------------------------------
struct TileDims { int ypitch, yrows, cpitch, crows; size_t lds; };
size_t tables_bytes(int th);
TileDims tile_dims(const DTick &T, const DLayer &L, int TH);
bool aligned16(const DPlane &p);

// ---- tick_bgra_stream (kernels_stream.hip.cpp) -------------------------------------------------------------------------------------------
bool stream_plane_ok(const DPlane &p);
bool bgra_stream_eligible(const DTick *ticks, const DLayer *layers, int n_ticks);

// ---- tick_yuv_stream (kernels_stream_yuv.hip.cpp) ----------------------------------------------------------------------------------------
bool ys_plane_ok(const DPlane &p);
bool ys_kind_rgb(int k);
// source classes of a launch (template parameter KINDS) and the LDS a wave needs for its widest tick
struct YsPlan { int kinds, nl, wave_bytes; };
YsPlan ys_plan(const DTick *ticks, const DLayer *layers, int n_ticks);
void ys_round(int tf, YsPlan &p);                // the instantiation a launch runs: (kinds, layers) rounded up to what is compiled
int ys_wave_bytes(const YsPlan &p, const DTick *ticks, const DLayer *layers, int n_ticks);
bool yuv_stream_eligible(int tf, const DTick *ticks, const DLayer *layers, int n_ticks, bool transient);

// ---- the strip kernels (kernels_wave.hip.cpp, kernels_wave_yuv.hip.cpp) -------------------------------------------------------------------
bool aligned16w(const DPlane &p);
bool host_src_rgb(int kind);
bool host_src_planar(int kind);
bool host_src_nv12(int kind);
struct WaveDims { int p0pitch, p0rows, p1pitch, p1rows; };
int strip_rows(int);
WaveDims wave_dims(const DTick &T, const DLayer &L, int WTH);
size_t wave_lds(const WaveDims &d, bool planar, int target_format, int rows);
// tail: the launch continues on canvases another launch has composed (the second part of a split batch)
bool wave_layers_eligible(int target_format, const DTick *ticks, const DLayer *layers, int n_ticks, bool tail = false);
// what the geometry tables were built for: any difference rebuilds them (strip height and LDS layout are chosen per LAUNCH, plan_wave_layers)
struct GeomConfig {
    int32_t target_format, wth, p0pitch, p0rows, p1pitch, p1rows, planar_any, strips_x, strips_y, n_layers;
    bool operator==(const GeomConfig &o) const {
        return target_format == o.target_format && wth == o.wth && p0pitch == o.p0pitch && p0rows == o.p0rows && p1pitch == o.p1pitch && p1rows == o.p1rows &&
               planar_any == o.planar_any && strips_x == o.strips_x && strips_y == o.strips_y && n_layers == o.n_layers;
    }
};
// What a launch of the strip kernels is shaped like — strip height, LDS layout, source classes — from its descriptors alone
struct WavePlan { int WTH; WaveDims m; bool planar; int kinds, side; size_t lds; };
WavePlan plan_wave_layers(int target_format, const DTick *ticks_host, const DLayer *layers_host, int n_ticks, int maxW, int maxH);
GeomConfig plan_config(const WavePlan &P, int target_format, int maxW, int maxH, int n_layers_total);
// the configuration launch_wave_layers will launch these ticks with; false: a launch that takes no tables (RGB layers only, or nothing staged)
bool wave_geom_config(int target_format, const DTick *ticks_host, const DLayer *layers_host, int n_ticks, int maxW, int maxH, int n_layers_total,
                      GeomConfig *cfg);
// may this lone tick travel as a kernel argument of the strip kernels (launch_transient)?
bool wave_layers_by_value(int target_format, const DTick *tick_host, const DLayer *layers_host);

}  // namespace chv
