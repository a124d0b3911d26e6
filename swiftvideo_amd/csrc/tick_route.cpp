// tick_route.cpp — which kernel runs a compositing tick: select_fast_path and everything it asks, the strip kernels'
// launch plan (plan_wave_layers: the routing and the geometry store need it before anything is launched) and the route names.  Pure host
// arithmetic on DTick, DLayer and the switches: no GPU compiler, no device header.  Every rule is pinned on the CPU by
// tests/cpp/test_tick_route.cpp (tests/test_tick_route.py); the launchers in the kernel units size their grids and LDS themselves and call
// tile_dims, ys_plan / ys_round / ys_wave_bytes and plan_wave_layers through tick_route.h.
#include "tick_route.h"
#include "switches.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

// the predicates compare doubles against bounds: no fused multiply-adds (the build's -ffp-contract=off says the same)
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace chv {

using namespace fast_path_ids;

bool finite16(const float *m) {
    for (int i = 0; i < 16; i++) if (!(m[i] - m[i] == 0.f)) return false;
    return true;
}

// ---------------------------------------------------------------------------
// the tiled kernel (kernels_fast.hip.cpp)
// ---------------------------------------------------------------------------
size_t tables_bytes(int th) { return th == TH_LARGE ? tile_tables_bytes(TH_LARGE) : tile_tables_bytes(TH_SMALL); }

// LDS rectangle one tile of this layer can touch, from the layer's scale factors.
TileDims tile_dims(const DTick &T, const DLayer &L, int TH) {
    const float *U = L.u;
    // |d(uv)/d(pixel)| as a fraction of the source per output pixel
    double sxr = std::fabs((double)U[U_TEXTURE + 0] * (double)U[U_TRANSFORM + 0] * 2.0 / (double)T.W);
    double syr = std::fabs((double)U[U_TEXTURE + 5] * (double)U[U_TRANSFORM + 5] * 2.0 / (double)T.H);
    TileDims d;
    int yspan = (int)std::ceil(TW * sxr * L.src.pl[0].w) + 4;   // texels incl. tap 1 and rounding slack
    int cspan = (int)std::ceil(TW * sxr * L.src.pl[1].w) + 4;
    d.ypitch = ((yspan + 15) / 16 + 3) * 16;                    // luma bytes: vectors + alignment + 2 pad vectors
    const bool planar = L.kind == LK_BGRA_FROM_Y420P;
    d.cpitch = planar ? ((cspan + 15) / 16 + 3) * 16 : ((cspan + 7) / 8 + 3) * 16;   // chroma bytes: U and V tiles (planar) / (u, v) pairs (NV12)
    // rows a tile's taps span: <= ceil((TH-1)*scale) + 2 (tap 1 of the last row) <= ceil(TH*scale) + 2
    d.yrows = (int)std::ceil(TH * syr * L.src.pl[0].h) + 3;
    d.crows = (int)std::ceil(TH * syr * L.src.pl[1].h) + 3;
    d.lds = tables_bytes(TH) + (size_t)d.ypitch * d.yrows + (size_t)d.cpitch * d.crows * (planar ? 2 : 1);
    return d;
}

// what the staged loads need: 16-byte aligned base and pitch, rows of at least one 16-byte vector
bool aligned16(const DPlane &p) { return (((uintptr_t)p.ptr) & 15) == 0 && (p.pitch & 15) == 0 && p.w * p.comps >= 16; }

const char *fast_path_name(int path) {
    switch (path) {
    case FP_NV12_BGRA_TILED: return "tick_nv12_bgra_tiled";
    case FP_Y420P_BGRA_TILED: return "tick_y420p_bgra_tiled";
    case FP_WAVE_LAYERS: return "tick_bgra_wave";
    case FP_STREAM: return "tick_bgra_stream";
    case FP_CLEAR_BGRA: return "canvas_clear_bgra";
    case FP_WAVE_NV12: return "tick_yuv_wave<nv12>";
    case FP_WAVE_Y420P: return "tick_yuv_wave<y420p>";
    case FP_STREAM_NV12: return "tick_yuv_stream<nv12>";
    case FP_STREAM_Y420P: return "tick_yuv_stream<y420p>";
    default: return "none";
    }
}

// the single-purpose kernel: exactly one YUV layer per tick (cfg2 / cfg4): block-tiled, strips of four tiles with the next
// tile's rectangle prefetched — 0.40-0.46 ms per 256 cfg2 ticks against 0.78 for the wave-per-strip kernel.  (RGB-only ticks
// had a block-tiled kernel of their own until the wave kernel overtook it: cfg3 1.92 vs 2.23 ms, cfg5 3.36 vs 3.67.)
int select_single_purpose(const DTick *ticks, const DLayer *layers, int n_ticks) {
    for (int i = 0; i < n_ticks; i++) {
        const DTick &T = ticks[i];
        if (T.n_layers != 1 || T.clear_first != ticks[0].clear_first) return FP_NONE;
        const DLayer &L = layers[T.first_layer];
        if ((L.kind != LK_BGRA_FROM_NV12 && L.kind != LK_BGRA_FROM_Y420P) || !(L.flags & LF_AXIS_ALIGNED)) return FP_NONE;
        if (L.kind != layers[ticks[0].first_layer].kind) return FP_NONE;
        if (!csc_absorbable(L.csc) && switches().bgra_path.load(std::memory_order_relaxed) != 2) return FP_NONE;      // (its fast rows need the absorbed matrix: the strip kernel is the faster one there)
        if (L.kind == LK_BGRA_FROM_Y420P && !aligned16(L.src.pl[2])) return FP_NONE;
        if (!finite16(L.u + U_TRANSFORM) || !finite16(L.u + U_TEXTURE) || !finite16(L.u + U_BORDER)) return FP_NONE;
        if (!aligned16(T.dst.pl[0]) || !aligned16(L.src.pl[0]) || !aligned16(L.src.pl[1])) return FP_NONE;
        if (tile_dims(T, L, TH_SMALL).lds > (size_t)LDS_BUDGET) return FP_NONE;
    }
    return layers[ticks[0].first_layer].kind == LK_BGRA_FROM_Y420P ? FP_Y420P_BGRA_TILED : FP_NV12_BGRA_TILED;
}

int select_fast_path(int target_format, const DTick *ticks, const DLayer *layers, int n_ticks, bool transient) {
    if (n_ticks <= 0) return FP_NONE;
    // A/B switches for measurements and tests (switches.h: environment read once, chv_debug_set_switch afterwards):
    //   force_general (CHV_FORCE_GENERAL=1)  everything through the general kernels
    //   bgra_path (CHV_BGRA_PATH=wave)       BGRA canvases: the wave-per-strip kernel also where the single-purpose kernel (exactly
    //                                        one YUV layer per tick) would be chosen;  =tiled: the single-purpose kernel wherever it applies
    const int bp = switches().bgra_path.load(std::memory_order_relaxed);
    if (switches().force_general.load(std::memory_order_relaxed)) return FP_NONE;
    // 4:2:0 canvases (the reference's own kernels): one wave per strip, or the general quad kernel
    // 4:2:0 canvases: cleared ticks of 1..4 axis-aligned layers without fill paint can stream their source rows (kernels_stream_yuv.hip.cpp: rows
    // outermost, a ring per layer, launches of every size); by default where that measured faster, everything else keeps the strip kernel
    if (target_format != TF_BGRA) {
        // Lone ticks of video layers from 720p up go to the strip kernel since ITS descriptors travel as a kernel argument too (WaveOne): 19.3 /
        // 20.3 / 30.6 us per 720p / 1080p / 2160p tick with the host wait against 20.5 / 22.5 / 35.7 through the rings; at 360p the streaming
        // kernel's short chunks keep it ahead (17.8 against 19.0), and the encoder side's integer frames are level (profiles/r06_notes.md section 15).
        // (Asked before the streaming kernel's own, longer list of conditions: where the strips can take such a tick they do either way.)
        if (transient && n_ticks == 1 && switches().yuv_stream.load(std::memory_order_relaxed) == 1 && (long)ticks[0].W * ticks[0].H >= 500000 &&
            ticks[0].n_layers >= 1 && ticks[0].n_layers <= WAVE_ONE_LAYERS && ticks[0].clear_first) {
            bool video_only = true;
            for (int l = 0; l < ticks[0].n_layers; l++) {
                const int k = layers[ticks[0].first_layer + l].kind;
                video_only = video_only && (k == LK_YUV_FROM_NV12 || k == LK_YUV_FROM_Y420P);
            }
            if (video_only && wave_layers_eligible(target_format, ticks, layers, n_ticks)) return target_format == TF_NV12 ? FP_WAVE_NV12 : FP_WAVE_Y420P;
        }
        if (yuv_stream_eligible(target_format, ticks, layers, n_ticks, transient)) return target_format == TF_NV12 ? FP_STREAM_NV12 : FP_STREAM_Y420P;
    }
    if (target_format != TF_BGRA)
        return wave_layers_eligible(target_format, ticks, layers, n_ticks) ? (target_format == TF_NV12 ? FP_WAVE_NV12 : FP_WAVE_Y420P) : FP_NONE;
    // ticks of 2..4 full-frame NV12 layers of one geometry on a cleared canvas: rows outermost, layers innermost (kernels_stream.hip.cpp);
    // one-layer ticks: a transient launch (chv_composite / chv_run_kernel: 19.7 against 22.6 us with the host wait through the tiled kernel —
    // its descriptors travel as kernel arguments, tools/tick_rows_sweep.sh; a one-tick BATCH reads them through pointers and is level with
    // the tiled kernel, which keeps it), otherwise on request (CHV_BGRA_PATH=stream; cfg2's 256-tick launches: 0.55 against 0.44 ms).
    // Launches of every size: the streaming kernel takes its chunk height as an
    // argument, and with 4-row chunks a lone 720p tick is 10.9 us on the chip against ~17 through 8-row strips of the strip kernel
    // (26.4 against 33.7 us per tick with the host wait; tools/tick_rows_sweep.sh, tools/stream_threshold_sweep.sh).
    if (transient && n_ticks == 1 && ticks[0].n_layers == 0 && ticks[0].clear_first && (((uintptr_t)ticks[0].dst.pl[0].ptr) & 3) == 0 &&
        (ticks[0].dst.pl[0].pitch & 3) == 0)
        return FP_CLEAR_BGRA;
    // A lone tick of ONE NV12 layer on a cleared canvas, now that the strip kernel has a twin that takes such a tick as a kernel argument
    // (tick_bgra_wave_one): the strips are ahead of the streaming kernel's twin on canvases from ~1.4 Mpixel up (a 1080p canvas: 20.8 against
    // 23.2 us with the host wait; at 720p the streaming kernel keeps it, 19.4 against 21.3) and of the tiled kernel's twin wherever the
    // streaming kernel does not apply (a picture-in-picture inset: 22.5 against 24.1 us at 720p, 21.2 against 23.4 at 1080p) —
    // tools/lone_bgra_routes.py.  Planar sources stay (their strip instantiation has no twin).
    const bool lone_nv12 = transient && bp == 0 && n_ticks == 1 && ticks[0].n_layers == 1 && ticks[0].clear_first &&
                           (layers[ticks[0].first_layer].kind == LK_BGRA_FROM_NV12 || layers[ticks[0].first_layer].kind == LK_BGRA_FROM_Y420P);
    if ((bp == 0 || bp == 3) && bgra_stream_eligible(ticks, layers, n_ticks)) {
        if (lone_nv12 && (long)ticks[0].W * ticks[0].H >= 1400000 && wave_layers_eligible(TF_BGRA, ticks, layers, n_ticks)) return FP_WAVE_LAYERS;
        if (bp == 3 || ticks[0].n_layers >= 2 || transient) return FP_STREAM;
    } else if (lone_nv12 && wave_layers_eligible(TF_BGRA, ticks, layers, n_ticks)) return FP_WAVE_LAYERS;
    if (bp != 1) {
        int p = select_single_purpose(ticks, layers, n_ticks);
        // planar sources in launches that fill the chip: the y420p-only instantiation of the wave kernel is the faster one
        // (cfg2_y420p 0.574 -> 0.532 ms; NV12 stays: 0.467 tiled vs 0.487 wave); small launches keep the tiled kernel's short strips
        if (p == FP_Y420P_BGRA_TILED && bp != 2) {
            long strips = 0;
            for (int i = 0; i < n_ticks; i++) strips += (long)((ticks[i].W + 63) / 64) * ((ticks[i].H + 15) / 16);
            if (strips >= 8192 && wave_layers_eligible(TF_BGRA, ticks, layers, n_ticks)) return FP_WAVE_LAYERS;
        }
        if (p != FP_NONE) return p;
    }
    // any mix of NV12 / y420p / BGRA / RGBA layers, any number of them.  (Launches that do not clear take the strip kernel also when ALL their
    // layers need its per-pixel path — rotated overlays added to composed canvases —: its grid covers the layers' boxes only, and measured
    // against the general kernel on the same boxes it is the faster one, 81 against 96 us for pipeline_logo's 128 rotated 320 x 180 logos.)
    return wave_layers_eligible(TF_BGRA, ticks, layers, n_ticks, !ticks[0].clear_first) ? FP_WAVE_LAYERS : FP_NONE;
}

// A batch whose ticks are "2..4 full-frame videos of one geometry, then something else" (a rotated logo, overlays, a fifth layer): how many
// leading layers of EVERY tick the streaming kernel takes as a launch of its own (cleared), the rest following in a second launch that continues
// on the canvas — the layer-by-layer semantics already are that (the canvas is re-quantised between layers either way).  0: no.
// The point: one layer the strip machinery has to apply per pixel (KINDS bit 3) otherwise puts the WHOLE tick on the strip kernel's most general
// instantiation (four waves per SIMD): the pipeline tick + a rotated logo 1.268 ms per 128 ticks against 0.62 for its four videos alone.
int split_stream_prefix(const DTick *ticks, const DLayer *layers, int n_ticks) {
    if (n_ticks < 1 || !switches().stream.load(std::memory_order_relaxed) || switches().bgra_path.load(std::memory_order_relaxed) != 0) return 0;
    if (switches().force_general.load(std::memory_order_relaxed)) return 0;
    int least = 1 << 30;
    for (int i = 0; i < n_ticks; i++) least = std::min(least, ticks[i].n_layers);
    std::vector<DTick> head(ticks, ticks + n_ticks);
    for (int k = std::min(4, least - 1); k >= 2; k--) {            // (every tick keeps at least one layer for the second launch)
        for (int i = 0; i < n_ticks; i++) head[(size_t)i].n_layers = k;
        if (bgra_stream_eligible(head.data(), layers, n_ticks)) return k;
    }
    return 0;
}
int fast_path_stream_bgra() { return FP_STREAM; }
// the path of a split batch's second launch
int select_tail_path(int target_format, const DTick *ticks, const DLayer *layers, int n_ticks) {
    const int p = select_fast_path(target_format, ticks, layers, n_ticks, false);
    if (p == FP_NONE && target_format == TF_BGRA && !switches().force_general.load(std::memory_order_relaxed) &&
        wave_layers_eligible(TF_BGRA, ticks, layers, n_ticks, true)) return FP_WAVE_LAYERS;
    return p;
}

bool fast_path_is_wave(int path) { return path == FP_WAVE_LAYERS || path == FP_WAVE_NV12 || path == FP_WAVE_Y420P; }
bool fast_path_by_value(int path) { return path == FP_STREAM || path == FP_STREAM_NV12 || path == FP_STREAM_Y420P || path == FP_NV12_BGRA_TILED || path == FP_Y420P_BGRA_TILED || path == FP_CLEAR_BGRA; }

// ---------------------------------------------------------------------------
// tick_bgra_stream (kernels_stream.hip.cpp)
// ---------------------------------------------------------------------------
bool stream_plane_ok(const DPlane &p) {
    return (((uintptr_t)p.ptr) & 15) == 0 && (p.pitch & 15) == 0 && ((p.w * p.comps) & 15) == 0 && p.w * p.comps >= 16 && p.h >= 1;
}

// every tick: cleared canvas, the same number (1..4) of NV12 -> BGRA layers of one geometry, axis-aligned and bounded, no flips, no fill,
// opacities in [0, 1], a strip's source columns within one 128-byte ring row
bool bgra_stream_eligible(const DTick *ticks, const DLayer *layers, int n_ticks) {
    if (n_ticks < 1 || !switches().stream.load(std::memory_order_relaxed)) return false;
    const int nl = ticks[0].n_layers;
    if (nl < 1 || nl > 4) return false;
    for (int i = 0; i < n_ticks; i++) {
        const DTick &T = ticks[i];
        if (T.n_layers != nl || !T.clear_first) return false;
        if ((((uintptr_t)T.dst.pl[0].ptr) & 3) != 0 || (T.dst.pl[0].pitch & 3) != 0) return false;
        for (int l = 0; l < nl; l++) {
            const DLayer &Y = layers[T.first_layer + l];
            // (NV12 or planar sources, one class per launch: LF_SAME_GEOM already says so inside a tick)
            const int kind0 = layers[ticks[0].first_layer].kind;
            if ((kind0 != LK_BGRA_FROM_NV12 && kind0 != LK_BGRA_FROM_Y420P) || Y.kind != kind0) return false;
            const bool planar = kind0 == LK_BGRA_FROM_Y420P;
            const int need = LF_AXIS_ALIGNED | LF_BOUNDED | LF_NO_FILL | (l ? LF_SAME_GEOM : 0);
            if ((Y.flags & need) != need) return false;
            const float op = Y.u[U_OPACITY];
            if (!(op >= 0.f && op <= 1.f)) return false;
            if (!stream_plane_ok(Y.src.pl[0]) || !stream_plane_ok(Y.src.pl[1])) return false;
            if (Y.src.pl[0].h > 32767 || Y.src.pl[1].h > 16383) return false;          // (the row table packs tap rows into 16 / 15 signed bits)
            if (Y.src.pl[1].comps != (planar ? 1 : 2) || Y.src.pl[0].comps != 1) return false;
            if (planar) {
                const DPlane &cu = Y.src.pl[1], &cv = Y.src.pl[2];
                if (!stream_plane_ok(cv) || cv.comps != 1 || cv.w != cu.w || cv.h != cu.h || cv.pitch != cu.pitch) return false;       // one ring geometry for U and V
            }
            if (l == 0) {
                // source texels per canvas pixel: u = (x / W * 2 - 1) * T0 * X0 + ...  =>  du/dx * w = 2 T0 X0 w / W
                const double kx = 2.0 * (double)Y.u[U_TRANSFORM + 0] * (double)Y.u[U_TEXTURE + 0], ky = 2.0 * (double)Y.u[U_TRANSFORM + 5] * (double)Y.u[U_TEXTURE + 5];
                if (!(kx > 0.0) || !(ky > 0.0)) return false;                                   // flips: the rings assume rising positions
                const double sx = kx * Y.src.pl[0].w / (double)T.W;
                if (!(63.0 * sx + 2.0 + 15.0 + 1.0 <= 128.0)) return false;                     // luma bytes of a strip (NV12 chroma: the same count)
                if (planar && !(63.0 * (kx * Y.src.pl[1].w / (double)T.W) + 2.0 + 15.0 + 1.0 <= (double)ST_CPP)) return false;     // a plane's chroma bytes of a strip
                // source rows per canvas row: the rings are advanced batch by batch (four luma rows per load), so the work per canvas row grows
                // with the vertical reduction — a picture squeezed into a few canvas rows (a zoom animation's first frames) would issue
                // hundreds of loads of rows nobody taps per canvas row, and tick_bgra_wave culls by bounding box instead
                const double sy = ky * Y.src.pl[0].h / (double)T.H;
                if (!std::isfinite(sy) || sy > 4.0) return false;
            }
        }
    }
    return true;
}

// ---------------------------------------------------------------------------
// tick_yuv_stream (kernels_stream_yuv.hip.cpp)
// ---------------------------------------------------------------------------
bool ys_plane_ok(const DPlane &p) {
    return p.ptr && (((uintptr_t)p.ptr) & 15) == 0 && (p.pitch & 15) == 0 && ((p.w * p.comps) & 15) == 0 && p.w * p.comps >= 16 && p.h >= 1 && p.h <= 8190 &&
           (long)p.pitch * p.h < (1L << 31);
}
bool ys_kind_rgb(int k) { return k == LK_YUV_FROM_RGB || k == LK_YUV_FROM_RGB_INT; }

YsPlan ys_plan(const DTick *ticks, const DLayer *layers, int n_ticks) {
    YsPlan p{ 0, 1, 0 };
    for (int i = 0; i < n_ticks; i++) {
        p.nl = std::max(p.nl, ticks[i].n_layers);
        for (int l = 0; l < ticks[i].n_layers; l++) {
            const int k = layers[ticks[i].first_layer + l].kind;
            p.kinds |= k == LK_YUV_FROM_NV12 ? YK_NV12 : k == LK_YUV_FROM_Y420P ? YK_PLANAR : k == LK_YUV_FROM_RGB ? YK_RGB : YK_RGBINT;
        }
    }
    return p;
}
// the instantiation a launch runs: (kinds, layers) rounded up to what is compiled
void ys_round(int tf, YsPlan &p) {
    const int own = tf == TF_NV12 ? YK_NV12 : YK_PLANAR;
    if (p.kinds == own) p.nl = p.nl <= 1 ? 1 : p.nl <= 2 ? 2 : 4;
    else if (p.kinds == YK_RGBINT && p.nl == 1) { }
    else if ((p.kinds & ~(own | YK_RGB)) == 0) { p.kinds = own | YK_RGB; p.nl = p.nl <= 3 ? 3 : 4; }
    else { p.kinds = YK_NV12 | YK_PLANAR | YK_RGB | YK_RGBINT; p.nl = 4; }
    if (p.kinds == own && p.nl == 4) { p.kinds = own | YK_RGB; }
}
int ys_wave_bytes(const YsPlan &p, const DTick *ticks, const DLayer *layers, int n_ticks) {
    const int nb = ys_rgb_b(p.kinds);
    int rings = 0;
    for (int i = 0; i < n_ticks; i++) {
        int r = 0;
        for (int l = 0; l < ticks[i].n_layers; l++) {
            const int k = layers[ticks[i].first_layer + l].kind;
            // (the kernel's own rule: a launch without RGB kinds / without YUV kinds never asks the layer)
            const bool rgb = (p.kinds & (YK_RGB | YK_RGBINT)) && (!(p.kinds & (YK_NV12 | YK_PLANAR)) || ys_kind_rgb(k));
            const bool planar = !rgb && (p.kinds & YK_PLANAR) && (!(p.kinds & YK_NV12) || k == LK_YUV_FROM_Y420P);
            r += ys_layer_bytes_c(rgb, planar, nb);
        }
        rings = std::max(rings, r);
    }
    return rings + p.nl * YS_TAB_BYTES;
}

// transient: one tick, launched once (chv_composite / chv_run_kernel)
bool yuv_stream_eligible(int tf, const DTick *ticks, const DLayer *layers, int n_ticks, bool transient) {
    const int mode = switches().yuv_stream.load(std::memory_order_relaxed);
    if (n_ticks < 1 || !mode) return false;
    if (tf != TF_NV12 && tf != TF_Y420P) return false;
    if (mode == 1) {
        // Where the streaming kernel is the faster one today (profiles/r04_notes.md; same-call A/Bs against tick_yuv_wave):
        //   * launches whose layers are all integer-matrix RGB pictures — the encoder side's full-frame conversion: 0.567 against 0.640 ms per
        //     128 frames of 1080p BGRA -> NV12, a lone frame 13.3 against 16.7 us;
        //   * lone ticks of video layers only (descriptors as kernel arguments, 4- to 16-row chunks): 13.9 against 15.4 us for a 1080p tick.
        // Batches of video layers are level (0.378 against 0.354 ms per 128 ticks) and stay with the strip kernel; ticks with float RGB
        // overlays are slower through the rings (a 1080p mixer tick: 31.8 against 21.4 us; 1.08 against 0.65 ms per 128) and stay there too.
        bool all_int = true, any_rgb = false;
        for (int i = 0; i < n_ticks; i++)
            for (int l = 0; l < ticks[i].n_layers; l++) {
                const int k = layers[ticks[i].first_layer + l].kind;
                all_int = all_int && k == LK_YUV_FROM_RGB_INT;
                any_rgb = any_rgb || k == LK_YUV_FROM_RGB || k == LK_YUV_FROM_RGB_INT;
            }
        if (!(all_int || (transient && n_ticks == 1 && !any_rgb))) return false;
    }
    for (int i = 0; i < n_ticks; i++) {
        const DTick &T = ticks[i];
        if (!T.clear_first || T.n_layers < 1 || T.n_layers > YS_MAXL) return false;
        if ((T.W & 7) || (T.H & 3) || T.W < 8 || T.H < 4 || T.dst.pl[0].w != T.W || T.dst.pl[0].h != T.H) return false;
        const int np = tf == TF_NV12 ? 2 : 3;
        for (int p = 0; p < np; p++) {
            const DPlane &P = T.dst.pl[p];
            if (!P.ptr || (((uintptr_t)P.ptr) & 3) || (P.pitch & 3)) return false;
            if (p > 0 && (P.w != T.W / 2 || P.h != T.H / 2)) return false;
        }
        for (int l = 0; l < T.n_layers; l++) {
            const DLayer &Y = layers[T.first_layer + l];
            const bool rgb = ys_kind_rgb(Y.kind), nv12 = Y.kind == LK_YUV_FROM_NV12, planar = Y.kind == LK_YUV_FROM_Y420P;
            if (!(rgb || nv12 || planar)) return false;
            if (nv12 && tf != TF_NV12) return false;
            const int need = LF_AXIS_ALIGNED | LF_BOUNDED | LF_NO_FILL;
            if ((Y.flags & need) != need) return false;
            if (!(Y.u[U_OPACITY] - Y.u[U_OPACITY] == 0.f)) return false;
            const int npl = rgb ? 1 : nv12 ? 2 : 3;
            for (int p = 0; p < npl; p++) if (!ys_plane_ok(Y.src.pl[p])) return false;
            if (rgb && Y.src.pl[0].comps != 4) return false;
            if (!rgb && (Y.src.pl[0].comps != 1 || Y.src.pl[1].comps != (nv12 ? 2 : 1))) return false;
            if (planar && (Y.src.pl[2].w != Y.src.pl[1].w || Y.src.pl[2].h != Y.src.pl[1].h || Y.src.pl[2].pitch != Y.src.pl[1].pitch || Y.src.pl[2].comps != 1)) return false;
            // source texels per canvas pixel: u = (x / W * 2 - 1) * T0 * X0 + ...  =>  du/dx * w = 2 T0 X0 w / W
            const double kx = 2.0 * (double)Y.u[U_TRANSFORM + 0] * (double)Y.u[U_TEXTURE + 0], ky = 2.0 * (double)Y.u[U_TRANSFORM + 5] * (double)Y.u[U_TEXTURE + 5];
            if (!(kx > 0.0) || !(ky > 0.0)) return false;                                   // flips: the rings assume rising positions
            const double sxr = kx * Y.src.pl[0].w / (double)T.W, syr = ky * Y.src.pl[0].h / (double)T.H;
            // An 8-row step asks the 24-row luma ring for the rows ry(row 0) .. ry(row 7) + 1, and ring_ensure holds hi - lo <= ROWS - B = 16:
            // ry(7) - ry(0) <= ceil(7 * syr) must stay <= 15, i.e. syr < 15 / 7 = 2.143 (at 2.2 a step could span 17 rows and row 7 would tap a
            // slot already holding the row 24 below: stale luma).  2.1 is the bound the fixed cases and the fuzzers exercise.
            if (!std::isfinite(sxr) || !std::isfinite(syr) || syr > 2.1) return false;
            // bytes of a ring row a strip's taps span: 63 steps + tap 1 + rounding slack, the start's alignment
            if (rgb) { if (!((63.0 * sxr + 3.0) * 4.0 + 12.0 <= 320.0)) return false; }
            else {
                if (!(63.0 * sxr + 3.0 + 15.0 <= 128.0)) return false;                      // luma; NV12 chroma: half the texels, two bytes each
                const double sxc = kx * Y.src.pl[1].w / (double)T.W;
                if (nv12 && !((63.0 * sxc + 3.0) * 2.0 + 14.0 <= 128.0)) return false;
                if (planar && !(63.0 * sxc + 3.0 + 15.0 <= 96.0)) return false;
            }
        }
    }
    YsPlan p = ys_plan(ticks, layers, n_ticks);
    ys_round(tf, p);
    // (a wave's rings and tables: beyond 16 KB the LDS holds fewer than ten waves per CU, and the strip kernel is the better choice)
    return ys_wave_bytes(p, ticks, layers, n_ticks) <= 16 * 1024;
}

// ---------------------------------------------------------------------------
// the strip kernels (kernels_wave.hip.cpp, kernels_wave_yuv.hip.cpp): eligibility and the launch plan of both
// ---------------------------------------------------------------------------
// (pitch < 2^24: the staging address arithmetic uses 24-bit multiplies)
bool aligned16w(const DPlane &p) { return (((uintptr_t)p.ptr) & 15) == 0 && (p.pitch & 15) == 0 && p.w * p.comps >= 16 && p.pitch < (1 << 24) && p.h < (1 << 24); }
bool host_src_rgb(int kind) { return kind == LK_BGRA_FROM_RGB || kind == LK_YUV_FROM_RGB || kind == LK_YUV_FROM_RGB_INT; }
bool host_src_planar(int kind) { return kind == LK_BGRA_FROM_Y420P || kind == LK_YUV_FROM_Y420P; }
bool host_src_nv12(int kind) { return kind == LK_BGRA_FROM_NV12 || kind == LK_YUV_FROM_NV12; }

int strip_rows(int) { return 8; }      // (the height every eligible tick must fit; launches may pick 16, see plan_wave_layers)

// LDS rectangles one strip of this layer can touch, from the layer's scale factors
WaveDims wave_dims(const DTick &T, const DLayer &L, int WTH) {
    const float *U = L.u;
    double sxr = std::fabs((double)U[U_TEXTURE + 0] * (double)U[U_TRANSFORM + 0] * 2.0 / (double)T.W);
    double syr = std::fabs((double)U[U_TEXTURE + 5] * (double)U[U_TRANSFORM + 5] * 2.0 / (double)T.H);
    WaveDims d{ 0, 0, 0, 0 };
    const bool rgb = host_src_rgb(L.kind), planar = host_src_planar(L.kind);
    const int bpt0 = rgb ? 4 : 1;
    int span0 = (int)std::ceil(WTW * sxr * L.src.pl[0].w) + 4;           // texels incl. tap 1 and rounding slack
    d.p0pitch = ((span0 * bpt0 + 15) / 16 + 3) * 16;                      // vectors + alignment + 2 pad vectors
    // (rectangles taller than two rows per strip row are staged as the rows' own tap-row pairs: WGeom::pair, wave_common.hip.h)
    d.p0rows = std::min((int)std::ceil(WTH * syr * L.src.pl[0].h) + CHV_P0ROWS_SLACK, (CHV_WAVE_PAIR && WTH == 8) ? 2 * WTH : (1 << 30));
    if (!rgb) {
        const int bpt1 = planar ? 1 : 2;
        int span1 = (int)std::ceil(WTW * sxr * L.src.pl[1].w) + 4;
        d.p1pitch = ((span1 * bpt1 + 15) / 16 + 3) * 16;
        d.p1rows = std::min((int)std::ceil(WTH * syr * L.src.pl[1].h) + 3, (CHV_WAVE_PAIR && WTH == 8) ? 2 * WTH : (1 << 30));
    }
    return d;
}
size_t wave_lds(const WaveDims &d, bool planar, int /*target_format*/, int rows) {
    return            (size_t)WAVES * ((size_t)rows * 48 + (size_t)d.p0pitch * d.p0rows + (size_t)d.p1pitch * d.p1rows * (planar ? 2 : 1));
}

// tail: the launch continues on canvases another launch has composed (the second part of a split batch): strips no layer touches leave at once,
// so the strip kernel is the better choice also where every layer needs the per-pixel path
bool wave_layers_eligible(int target_format, const DTick *ticks, const DLayer *layers, int n_ticks, bool tail) {
    bool any_general = false, any_staged = false;
    for (int i = 0; i < n_ticks; i++) {
        const DTick &T = ticks[i];
        if (T.n_layers < 1 || T.clear_first != ticks[0].clear_first) return false;
        if (target_format == TF_BGRA) {
            if (!aligned16w(T.dst.pl[0])) return false;
        } else {
            // 4:2:0: even canvas, chroma planes exactly half size (odd sizes, where gid/2 leaves the chroma plane, stay on the general kernel)
            const int np = target_format == TF_NV12 ? 2 : 3;
            if ((T.W & 1) || (T.H & 1) || T.dst.pl[0].w != T.W || T.dst.pl[0].h != T.H) return false;
            for (int p = 1; p < np; p++) if (T.dst.pl[p].w != T.W / 2 || T.dst.pl[p].h != T.H / 2) return false;
        }
        for (int l = 0; l < T.n_layers; l++) {
            const DLayer &L = layers[T.first_layer + l];
            const bool rgb = host_src_rgb(L.kind), nv12 = host_src_nv12(L.kind), planar = host_src_planar(L.kind);
            // img_bgra_bgra (kernels.metal:52-62 — what an unchanged VideoMixer.findKernel resolves a BGRA layer on a BGRA canvas to):
            // nearest sampling, nothing to stage; applied per pixel inside the wave kernel like a rotated layer, so that a
            // reference-default tick of video layers + a BGRA overlay keeps the strip path for its video layers
            if (L.kind == LK_BGRA_METAL && target_format == TF_BGRA) { any_general = true; continue; }
            if (!(rgb || nv12 || planar)) return false;
            // layers that cannot be staged (rotation, shear, unbounded matrices) are applied per pixel inside the kernel: nothing to check
            if ((L.flags & (LF_AXIS_ALIGNED | LF_BOUNDED)) != (LF_AXIS_ALIGNED | LF_BOUNDED)) { any_general = true; continue; }
            any_staged = true;
            if (!finite16(L.u + U_TRANSFORM) || !finite16(L.u + U_TEXTURE) || !finite16(L.u + U_BORDER)) return false;
            const int np = rgb ? 1 : nv12 ? 2 : 3;
            for (int p = 0; p < np; p++) if (!aligned16w(L.src.pl[p])) return false;
            if (planar && (L.src.pl[2].w != L.src.pl[1].w || L.src.pl[2].h != L.src.pl[1].h)) return false;   // one staging geometry for U and V
            if (wave_lds(wave_dims(T, L, strip_rows(target_format)), planar, target_format, strip_rows(target_format)) > (size_t)LDS_BUDGET) return false;
        }
    }
    // (a launch whose layers ALL need the per-pixel path gains nothing here: the general kernel it is)
    return any_staged || !any_general || tail;
}

// What a launch of the strip kernels is shaped like — strip height, LDS layout, source classes — from its descriptors alone (launch_wave_layers
// launches with it; the store asks for it through wave_geom_config before the descriptors go to the device: the tables it looks up were built
// for one shape).
WavePlan plan_wave_layers(int target_format, const DTick *ticks_host, const DLayer *layers_host, int n_ticks, int maxW, int maxH) {
    // Strip height.  16 rows when the launch has enough strips to fill the chip's wave slots with them and the taller
    // rectangles leave room for two strips per 64 KB of LDS; on BGRA canvases (whose 16-row instantiation has no masked rows:
    // registers) only when every layer covers (almost) the whole canvas, so that hardly any strip is crossed by a layer's
    // edge.  8 rows otherwise.  CHV_WAVE_ROWS=8|16 is the A/B and test switch.
    int WTH = strip_rows(target_format);
    {
        const int forced = switches().wave_rows.load(std::memory_order_relaxed);
        bool tall = (long)n_ticks * ((maxW + WTW - 1) / WTW) * ((maxH + 15) / 16) >= 8192;
        if (target_format == TF_BGRA) {
            for (int i = 0; i < n_ticks && tall; i++) {
                const DTick &T = ticks_host[i];
                for (int l = 0; l < T.n_layers && tall; l++) {
                    const int32_t *bb = layers_host[T.first_layer + l].bbox;
                    tall = (double)(bb[2] - bb[0]) * (double)(bb[3] - bb[1]) >= 0.9 * (double)T.W * (double)T.H;
                }
            }
        }
        if (forced == 8 || forced == 16) tall = forced == 16;
        if (tall) WTH = 16;
    }
    WaveDims m{ 0, 0, 0, 0 };
    bool planar = false;
    int kinds = 0;               // source classes in the launch: bit 0 NV12, bit 1 y420p, bit 2 RGB
    auto measure = [&](int rows) {
        m = WaveDims{ 0, 0, 0, 0 };
        planar = false;
        for (int i = 0; i < n_ticks; i++) {
            for (int l = 0; l < ticks_host[i].n_layers; l++) {
                const DLayer &L = layers_host[ticks_host[i].first_layer + l];
                if (L.kind == LK_BGRA_METAL || (L.flags & (LF_AXIS_ALIGNED | LF_BOUNDED)) != (LF_AXIS_ALIGNED | LF_BOUNDED)) { kinds |= 8; continue; }     // not staged
                WaveDims d = wave_dims(ticks_host[i], L, rows);
                m.p0pitch = std::max(m.p0pitch, d.p0pitch); m.p0rows = std::max(m.p0rows, d.p0rows);
                m.p1pitch = std::max(m.p1pitch, d.p1pitch); m.p1rows = std::max(m.p1rows, d.p1rows);
                planar = planar || host_src_planar(L.kind);
                kinds |= host_src_rgb(L.kind) ? 4 : host_src_planar(L.kind) ? 2 : 1;
            }
        }
        return wave_lds(m, planar, target_format, rows);
    };
    size_t lds = measure(WTH);
    if (WTH == 16 && lds > (size_t)LDS_BUDGET / 2) { WTH = 8; lds = measure(WTH); }      // (keep at least two tall strips' worth per 64 KB)
    // Side-by-side layout: a YUV layer's luma, chroma / U and V rectangles next to each other in the rows of ONE region whose rows are as wide as the
    // widest need of the launch — an RGB rectangle (the mixer canvas: a video layer's 128 + 96 + 96 bytes in an overlay's 320) or luma + chroma of
    // the widest video layer — instead of a plane-0 region followed by chroma regions.  The region is then max(rows) x pitch instead of the sum of
    // the regions; taken where that is smaller (18 -> 23 waves' worth of LDS per CU on the mixer canvas, 20 -> 26 for video + overlays on BGRA).
    int side = 0;
    if ((kinds & 3) && lds <= (size_t)LDS_BUDGET) {
        int yneed = 0, c_nv12 = 0, c_planar = 0;
        for (int i = 0; i < n_ticks; i++)
            for (int l = 0; l < ticks_host[i].n_layers; l++) {
                const DLayer &L = layers_host[ticks_host[i].first_layer + l];
                if (L.kind == LK_BGRA_METAL || (L.flags & (LF_AXIS_ALIGNED | LF_BOUNDED)) != (LF_AXIS_ALIGNED | LF_BOUNDED) || host_src_rgb(L.kind)) continue;
                const WaveDims d = wave_dims(ticks_host[i], L, WTH);
                yneed = std::max(yneed, d.p0pitch);
                if (host_src_planar(L.kind)) c_planar = std::max(c_planar, d.p1pitch); else c_nv12 = std::max(c_nv12, d.p1pitch);
            }
        const int planes = planar ? 2 : 1;
        const int pitch = std::max(m.p0pitch, yneed + std::max(c_nv12, 2 * c_planar));
        const size_t separate = (size_t)m.p0pitch * m.p0rows + (size_t)m.p1pitch * m.p1rows * planes;
        const size_t beside = (size_t)pitch * std::max(m.p0rows, m.p1rows);
        if (yneed > 0 && beside < separate && (yneed >> 4) < 4096 && (c_planar >> 4) < 4096) {
            // bits 8-19: luma columns / 16; bits 20-31: columns of ONE planar chroma plane / 16 (0: no planar picture in the launch)
            side = ((yneed >> 4) << 8) | ((c_planar >> 4) << 20) | (1 << 7);
            m.p0pitch = pitch;
            lds = lds - (size_t)WAVES * separate + (size_t)WAVES * beside;
        }
    }
    if (lds > (size_t)LDS_BUDGET) {
        // per-layer maxima combined exceed the budget: shrink the row counts; rectangles that do not fit fall back to
        // unstaged taps inside the kernel
        const size_t fixed = (size_t)WAVES * WTH * 48;     // (row table: WaveCfg::ROWTAB_BYTES)
        const size_t per_row = (size_t)WAVES * ((size_t)m.p0pitch + (size_t)m.p1pitch * (planar ? 2 : 1));
        int rows = std::max(1, (int)((LDS_BUDGET - fixed) / per_row));
        m.p0rows = std::min(m.p0rows, rows); m.p1rows = std::min(m.p1rows, rows);
        lds = wave_lds(m, planar, target_format, WTH);
    }
#ifdef CHV_EXP_LDS_PAD
    // measurement-only variant (tools/build_variant.sh … -DCHV_EXP_LDS_PAD): extra LDS per block caps the waves per SIMD — how much
    // occupancy the strip kernels need (profiles/r03_notes.md section 7)
    if (const char *pad = getenv("CHV_LDS_PAD")) { fprintf(stderr, "[chv] lds %zu + pad %d, rows %d\n", lds, atoi(pad), WTH); lds += (size_t)atoi(pad); }
#endif
    m.p0rows = std::min(m.p0rows, 0xFFFF); m.p1rows = std::min(m.p1rows, 0xFFFF);      // (far beyond what LDS holds: such rectangles are not staged anyway)
    return WavePlan{ WTH, m, planar, kinds, side, lds };
}
GeomConfig plan_config(const WavePlan &P, int target_format, int maxW, int maxH, int n_layers_total) {
    return GeomConfig{ target_format, P.WTH, P.m.p0pitch, P.m.p0rows, P.m.p1pitch, P.m.p1rows, (P.planar ? 1 : 0) | P.side, (maxW + WTW - 1) / WTW, (maxH + P.WTH - 1) / P.WTH, n_layers_total };
}
bool wave_geom_config(int target_format, const DTick *ticks_host, const DLayer *layers_host, int n_ticks, int maxW, int maxH, int n_layers_total,
                      GeomConfig *cfg) {
    const WavePlan P = plan_wave_layers(target_format, ticks_host, layers_host, n_ticks, maxW, maxH);
    *cfg = plan_config(P, target_format, maxW, maxH, n_layers_total);
    return P.kinds != 4 && (P.kinds & 7) != 0;
}

// May this lone tick travel as a kernel argument (launch_transient: no descriptor slot, no copy)?  4:2:0 canvases: every instantiation of
// tick_yuv_wave takes one; BGRA canvases: tick_bgra_wave_one exists for cleared canvases, 8-row strips and launches without per-pixel layers.
bool wave_layers_by_value(int target_format, const DTick *tick_host, const DLayer *layers_host) {
    if (tick_host->n_layers < 1 || tick_host->n_layers > WAVE_ONE_LAYERS) return false;
    if (target_format != TF_BGRA) return true;
    if (!tick_host->clear_first) return false;
    const WavePlan P = plan_wave_layers(target_format, tick_host, layers_host, 1, tick_host->W, tick_host->H);
    return P.WTH == 8 && !(P.kinds & 8) && P.kinds != 4;
}

}  // namespace chv
