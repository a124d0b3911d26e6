// test_tick_route.cpp — which kernel runs a compositing tick, on the CPU (swiftvideo_amd/csrc/tick_route.cpp).  g++ only, no HIP:
// descriptors built in code, planes at fake 16-byte-aligned addresses that nothing dereferences, switches set per case through this
// program's own chv::switches().
//
// Every case has one line in tick_route_answers.inc: what select_fast_path (transient and batched), select_tail_path, split_stream_prefix,
// wave_layers_by_value, the four *_eligible predicates and wave_geom_config said at the commit BEFORE the rules moved into tick_route.cpp,
// when they lived in four kernel units — printed by tools/tick_route_diff.cpp (which includes this file for its cases) linked against that
// commit's library.  kYsRound was printed by ys_round's text of that commit.  The moved functions must go on saying what the units said.
//
// Bounds: where a rule's bound is a ratio of integers (63 sx + 18 <= 128 is sx <= 110 / 63), the case AT the bound uses a source and a canvas
// size whose quotient is that ratio, so the comparison sees the bound's own double; the case above it is the next admissible plane size.
#include "tick_route.h"
#include "switches.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace chv;
using namespace chv::fast_path_ids;

#ifndef TICK_ROUTE_DRIVER
// the switches the rules read (the library's own live in chipvideo.cpp)
Switches &chv::switches() {
    static Switches s;
    return s;
}
static void set_switch(std::atomic<int> Switches::*which, int value) { (switches().*which).store(value); }
#else
static void set_switch(std::atomic<int> Switches::*which, int value);      // (the driver: through chv_debug_set_switch)
#endif

namespace {

struct Scene {
    int tf;
    std::vector<DTick> t;
    std::vector<DLayer> l;
    // one more tick on its own canvas (W x H, cleared) with these layers
    Scene &tick(int W, int H, std::vector<DLayer> layers);
};

uint8_t *fake(int n) { return (uint8_t *)(uintptr_t)(0x40000000ull + (uint64_t)n * 0x04000000ull); }
DPlane plane(int n, int w, int h, int comps) { return DPlane{ fake(n), w, h, (w * comps + 15) & ~15, comps }; }

Scene &Scene::tick(int W, int H, std::vector<DLayer> layers) {
    DTick T = {};
    T.W = W; T.H = H; T.clear_first = 1;
    if (tf == TF_BGRA) T.dst.pl[0] = DPlane{ fake(1), W, H, W * 4, 4 };
    else {
        T.dst.pl[0] = DPlane{ fake(1), W, H, W, 1 };
        if (tf == TF_NV12) T.dst.pl[1] = DPlane{ fake(2), W / 2, H / 2, W, 2 };
        else { T.dst.pl[1] = DPlane{ fake(2), W / 2, H / 2, W / 2, 1 }; T.dst.pl[2] = DPlane{ fake(3), W / 2, H / 2, W / 2, 1 }; }
    }
    T.n_layers = (int)layers.size(); T.first_layer = (int)l.size();
    for (DLayer &L : layers) {
        if (L.bbox[2] < 0) { L.bbox[0] = 0; L.bbox[1] = 0; L.bbox[2] = W; L.bbox[3] = H; }
        l.push_back(L);
    }
    t.push_back(T);
    return *this;
}

// a layer of `kind` from a sw x sh picture (chroma planes half size, rounded up), axis aligned: kx, ky = 2 x transform x texture scale, i.e.
// source texels per canvas pixel = kx sw / W; bounding box: the canvas (bbox[2] < 0 until the tick is known)
DLayer layer(int kind, int sw, int sh, double kx = 1.0, double ky = 1.0, float opacity = 1.f) {
    DLayer L = {};
    L.kind = kind;
    const bool rgb = kind == LK_BGRA_FROM_RGB || kind == LK_YUV_FROM_RGB || kind == LK_YUV_FROM_RGB_INT || kind == LK_BGRA_METAL;
    const bool planar = kind == LK_BGRA_FROM_Y420P || kind == LK_YUV_FROM_Y420P;
    if (rgb) L.src.pl[0] = plane(8, sw, sh, 4);
    else {
        L.src.pl[0] = plane(8, sw, sh, 1);
        L.src.pl[1] = plane(9, (sw + 1) / 2, (sh + 1) / 2, planar ? 1 : 2);
        if (planar) L.src.pl[2] = plane(10, (sw + 1) / 2, (sh + 1) / 2, 1);
    }
    for (int d = 0; d < 4; d++) { L.u[U_TRANSFORM + 5 * d] = 1.f; L.u[U_TEXTURE + 5 * d] = 1.f; L.u[U_BORDER + 5 * d] = 1.f; }
    L.u[U_TEXTURE + 0] = (float)(kx / 2.0); L.u[U_TEXTURE + 5] = (float)(ky / 2.0);
    L.u[U_OPACITY] = opacity;
    L.flags = LF_AXIS_ALIGNED | LF_BOUNDED | LF_NO_FILL | (opacity == 1.f ? LF_OPAQUE : 0);
    L.bbox[2] = -1;
    return L;
}
DLayer same_geom(DLayer L) { L.flags |= LF_SAME_GEOM; return L; }
DLayer rotated(DLayer L) { L.flags &= ~LF_AXIS_ALIGNED; return L; }
DLayer with_chroma(DLayer L, int cw, int ch) {
    L.src.pl[1] = plane(9, cw, ch, L.src.pl[1].comps);
    if (L.src.pl[2].ptr) L.src.pl[2] = plane(10, cw, ch, 1);
    return L;
}
DLayer with_bbox(DLayer L, int x0, int y0, int x1, int y1) { L.bbox[0] = x0; L.bbox[1] = y0; L.bbox[2] = x1; L.bbox[3] = y1; return L; }

// everything the routing says about a scene, as one line
std::string answers(const Scene &s) {
    const int n = (int)s.t.size();
    const DTick *t = s.t.data();
    const DLayer *l = s.l.data();
    GeomConfig c = {};
    const bool takes = wave_geom_config(s.tf, t, l, n, t[0].W, t[0].H, (int)s.l.size(), &c);
    char buf[256];
    std::snprintf(buf, sizeof buf, "lone %d batch %d tail %d split %d by_value %d wave %d%d bgra_stream %d yuv_stream %d%d config %d %d/%d/%d/%d/%d 0x%x %dx%d",
                  n == 1 ? select_fast_path(s.tf, t, l, 1, true) : -9, select_fast_path(s.tf, t, l, n), select_tail_path(s.tf, t, l, n), split_stream_prefix(t, l, n),
                  (int)wave_layers_by_value(s.tf, t, l), (int)wave_layers_eligible(s.tf, t, l, n), (int)wave_layers_eligible(s.tf, t, l, n, true),
                  (int)bgra_stream_eligible(t, l, n), (int)yuv_stream_eligible(s.tf, t, l, n, n == 1), (int)yuv_stream_eligible(s.tf, t, l, n, false),
                  (int)takes, c.wth, c.p0pitch, c.p0rows, c.p1pitch, c.p1rows, (unsigned)c.planar_any, c.strips_x, c.strips_y);
    return buf;
}

void defaults() {
    set_switch(&Switches::force_general, 0); set_switch(&Switches::bgra_path, 0); set_switch(&Switches::wave_rows, 0);
    set_switch(&Switches::stream, 1); set_switch(&Switches::yuv_stream, 1);
}

// the cases: `emit(name, scene)` under the switches set just before
template <class Emit>
void cases(Emit emit) {
    const int NV = LK_YUV_FROM_NV12, PL = LK_YUV_FROM_Y420P, RGB = LK_YUV_FROM_RGB, INT = LK_YUV_FROM_RGB_INT;
    const int BNV = LK_BGRA_FROM_NV12, BPL = LK_BGRA_FROM_Y420P, BRGB = LK_BGRA_FROM_RGB;
    auto one = [](int tf, int W, int H, std::vector<DLayer> layers) { Scene s{ tf, {}, {} }; s.tick(W, H, layers); return s; };
    auto many = [](int tf, int n, int W, int H, std::vector<DLayer> layers) { Scene s{ tf, {}, {} }; for (int i = 0; i < n; i++) s.tick(W, H, layers); return s; };
    defaults();

    // ---- 4:2:0 canvas, lone video tick: 500 000 pixels, WAVE_ONE_LAYERS ----
    emit("420 lone nv12 992x504", one(TF_NV12, 992, 504, { layer(NV, 992, 504) }));
    emit("420 lone nv12 1000x500", one(TF_NV12, 1000, 500, { layer(NV, 1008, 500) }));
    emit("420 lone y420p 992x504", one(TF_Y420P, 992, 504, { layer(PL, 992, 504) }));
    emit("420 lone y420p 1000x500", one(TF_Y420P, 1000, 500, { layer(PL, 1008, 500) }));
    for (int nl : { 4, 5, WAVE_ONE_LAYERS, WAVE_ONE_LAYERS + 1 }) {
        char name[64];
        std::snprintf(name, sizeof name, "420 lone nv12 1000x500 %d layers", nl);
        emit(name, one(TF_NV12, 1000, 500, std::vector<DLayer>((size_t)nl, layer(NV, 1008, 500, 1.0, 1.0, 0.5f))));
    }
    // ---- CHV_YUV_STREAM 0 / 1 / force ----
    for (int mode = 0; mode <= 2; mode++) {
        set_switch(&Switches::yuv_stream, mode);
        const std::string m = " yuv_stream=" + std::to_string(mode);
        emit("420 batch of integer RGB" + m, many(TF_NV12, 3, 64, 32, { layer(INT, 64, 32) }));
        emit("420 batch of video" + m, many(TF_NV12, 3, 64, 32, { layer(NV, 64, 32), layer(NV, 32, 16, 1.0, 1.0, 0.5f) }));
        emit("420 y420p batch of video" + m, many(TF_Y420P, 2, 64, 32, { layer(PL, 64, 32) }));
        emit("420 lone video" + m, one(TF_NV12, 64, 32, { layer(NV, 64, 32) }));
        emit("420 lone video + float RGB overlay" + m, one(TF_NV12, 64, 32, { layer(NV, 64, 32), layer(RGB, 32, 16, 1.0, 1.0, 0.5f) }));
        emit("420 lone integer RGB" + m, one(TF_Y420P, 64, 32, { layer(INT, 64, 32) }));
    }
    // ---- yuv_stream_eligible, per-tick rules (forced, so that the rules decide) ----
    set_switch(&Switches::yuv_stream, 2);
    emit("ys syr 2.1", one(TF_NV12, 64, 40, { layer(NV, 64, 84) }));
    emit("ys syr above 2.1", one(TF_NV12, 64, 40, { layer(NV, 64, 86) }));
    emit("ys rgb ring at 320", one(TF_NV12, 1008, 8, { layer(RGB, 1184, 8) }));
    emit("ys rgb ring above", one(TF_NV12, 1008, 8, { layer(RGB, 1188, 8) }));
    emit("ys luma ring at 128", one(TF_NV12, 1008, 8, { with_chroma(layer(NV, 1760, 8), 800, 4) }));
    emit("ys luma ring above", one(TF_NV12, 1008, 8, { with_chroma(layer(NV, 1776, 8), 800, 4) }));
    emit("ys nv12 chroma ring at 128", one(TF_NV12, 1008, 8, { with_chroma(layer(NV, 1600, 8), 864, 4) }));
    emit("ys nv12 chroma ring above", one(TF_NV12, 1008, 8, { with_chroma(layer(NV, 1600, 8), 872, 4) }));
    emit("ys planar chroma ring at 96", one(TF_Y420P, 1008, 8, { with_chroma(layer(PL, 1600, 8), 1248, 4) }));
    emit("ys planar chroma ring above", one(TF_Y420P, 1008, 8, { with_chroma(layer(PL, 1600, 8), 1264, 4) }));
    emit("ys canvas W&7", one(TF_NV12, 68, 32, { layer(NV, 64, 32) }));
    emit("ys canvas H&3", one(TF_NV12, 64, 34, { layer(NV, 64, 32) }));
    emit("ys canvas 8x4", one(TF_NV12, 8, 4, { layer(NV, 16, 4) }));
    { Scene s = one(TF_NV12, 64, 32, { layer(NV, 64, 32) }); s.t[0].dst.pl[1].w = 31; emit("ys odd chroma plane", s); }
    emit("ys flip", one(TF_NV12, 64, 32, { layer(NV, 64, 32, -1.0, 1.0) }));
    emit("ys NaN opacity", one(TF_NV12, 64, 32, { layer(NV, 64, 32, 1.0, 1.0, NAN) }));
    { DLayer L = layer(NV, 64, 32); L.flags &= ~LF_NO_FILL; emit("ys fill paint", one(TF_NV12, 64, 32, { L })); }
    emit("ys nv12 picture on a y420p canvas", one(TF_Y420P, 64, 32, { layer(NV, 64, 32) }));
    emit("ys source rows 8190", one(TF_NV12, 64, 4096, { layer(NV, 64, 8190) }));
    emit("ys source rows 8192", one(TF_NV12, 64, 4096, { layer(NV, 64, 8192) }));
    // ---- yuv_stream_eligible, LDS: the 16 KB rule ----
    emit("ys 3 nv12 layers", one(TF_NV12, 64, 32, std::vector<DLayer>(3, layer(NV, 64, 32, 1.0, 1.0, 0.5f))));
    emit("ys 4 nv12 layers", one(TF_NV12, 64, 32, std::vector<DLayer>(4, layer(NV, 64, 32, 1.0, 1.0, 0.5f))));
    emit("ys 2 y420p + 1 rgb", one(TF_Y420P, 64, 32, { layer(PL, 64, 32), layer(PL, 64, 32, 1.0, 1.0, 0.5f), layer(RGB, 32, 16) }));
    emit("ys 2 y420p + 2 rgb", one(TF_Y420P, 64, 32, { layer(PL, 64, 32), layer(PL, 64, 32, 1.0, 1.0, 0.5f), layer(RGB, 32, 16), layer(RGB, 32, 16) }));
    emit("ys 4 rgb", one(TF_NV12, 64, 32, std::vector<DLayer>(4, layer(RGB, 64, 32, 1.0, 1.0, 0.5f))));
    emit("ys 5 rgb", one(TF_NV12, 64, 32, std::vector<DLayer>(5, layer(RGB, 64, 32, 1.0, 1.0, 0.5f))));
    defaults();

    // ---- BGRA canvas, routes ----
    { Scene s{ TF_BGRA, {}, {} }; s.tick(64, 32, {}); emit("bgra layerless lone clear", s); s.t[0].dst.pl[0].pitch = 258; emit("bgra layerless clear, pitch & 3", s); }
    emit("bgra lone nv12 1400x999", one(TF_BGRA, 1400, 999, { layer(BNV, 1408, 1000) }));
    emit("bgra lone nv12 1400x1000", one(TF_BGRA, 1400, 1000, { layer(BNV, 1408, 1000) }));
    emit("bgra lone y420p 1400x1000", one(TF_BGRA, 1400, 1000, { layer(BPL, 1408, 1000) }));
    // a picture-in-picture inset: the transform squeezes the picture, kx = 8 source texels per canvas pixel of a 64-wide picture on 256: too wide a ring row
    emit("bgra lone inset the stream kernel refuses", one(TF_BGRA, 256, 128, { with_bbox(layer(BNV, 512, 128, 4.0, 1.0), 64, 32, 128, 96) }));
    for (int bp = 0; bp <= 3; bp++) {
        set_switch(&Switches::bgra_path, bp);
        const std::string m = " bgra_path=" + std::to_string(bp);
        emit("bgra lone nv12" + m, one(TF_BGRA, 128, 64, { layer(BNV, 128, 64) }));
        emit("bgra batch nv12" + m, many(TF_BGRA, 3, 128, 64, { layer(BNV, 128, 64) }));
        emit("bgra batch y420p" + m, many(TF_BGRA, 3, 128, 64, { layer(BPL, 128, 64) }));
        emit("bgra batch 2 nv12" + m, many(TF_BGRA, 3, 128, 64, { layer(BNV, 128, 64), same_geom(layer(BNV, 128, 64, 1.0, 1.0, 0.5f)) }));
        { DLayer L = layer(BNV, 128, 64); L.csc = 2; emit("bgra batch nv12, BT.601 full range" + m, many(TF_BGRA, 3, 128, 64, { L })); }
        emit("bgra batch rgb" + m, many(TF_BGRA, 3, 128, 64, { layer(BRGB, 128, 64) }));
    }
    defaults();
    set_switch(&Switches::stream, 0);
    emit("bgra lone nv12 stream=0", one(TF_BGRA, 128, 64, { layer(BNV, 128, 64) }));
    emit("bgra batch 4 nv12 + logo stream=0", many(TF_BGRA, 2, 128, 64, { layer(BNV, 128, 64), same_geom(layer(BNV, 128, 64)), rotated(layer(BRGB, 32, 16)) }));
    defaults();
    set_switch(&Switches::force_general, 1);
    emit("bgra lone nv12 force_general", one(TF_BGRA, 128, 64, { layer(BNV, 128, 64) }));
    emit("420 lone nv12 force_general", one(TF_NV12, 64, 32, { layer(NV, 64, 32) }));
    emit("bgra batch 2 nv12 + logo force_general", many(TF_BGRA, 2, 128, 64, { layer(BNV, 128, 64), same_geom(layer(BNV, 128, 64)), rotated(layer(BRGB, 32, 16)) }));
    defaults();

    // ---- bgra_stream_eligible ----
    emit("bs sx at 110/63", many(TF_BGRA, 2, 1008, 8, { layer(BNV, 1760, 8), same_geom(layer(BNV, 1760, 8)) }));
    emit("bs sx above", many(TF_BGRA, 2, 1008, 8, { layer(BNV, 1776, 8), same_geom(layer(BNV, 1776, 8)) }));
    emit("bs planar chroma at ST_CPP", many(TF_BGRA, 2, 1008, 8, { with_chroma(layer(BPL, 1600, 8), 1248, 4), same_geom(with_chroma(layer(BPL, 1600, 8), 1248, 4)) }));
    emit("bs planar chroma above", many(TF_BGRA, 2, 1008, 8, { with_chroma(layer(BPL, 1600, 8), 1264, 4), same_geom(with_chroma(layer(BPL, 1600, 8), 1264, 4)) }));
    emit("bs sy 4.0", many(TF_BGRA, 2, 64, 8, { layer(BNV, 64, 32), same_geom(layer(BNV, 64, 32)) }));
    emit("bs sy above 4", many(TF_BGRA, 2, 64, 8, { layer(BNV, 64, 34), same_geom(layer(BNV, 64, 34)) }));
    emit("bs luma rows 32767", many(TF_BGRA, 2, 64, 8192, { with_chroma(layer(BNV, 64, 32767), 32, 16383), same_geom(with_chroma(layer(BNV, 64, 32767), 32, 16383)) }));
    emit("bs luma rows 32768", many(TF_BGRA, 2, 64, 8192, { with_chroma(layer(BNV, 64, 32768), 32, 16383), same_geom(with_chroma(layer(BNV, 64, 32768), 32, 16383)) }));
    emit("bs chroma rows 16384", many(TF_BGRA, 2, 64, 8192, { with_chroma(layer(BNV, 64, 32767), 32, 16384), same_geom(with_chroma(layer(BNV, 64, 32767), 32, 16384)) }));
    emit("bs layer 1 without LF_SAME_GEOM", many(TF_BGRA, 2, 128, 64, { layer(BNV, 128, 64), layer(BNV, 128, 64) }));
    emit("bs opacity 1.0", many(TF_BGRA, 2, 128, 64, { layer(BNV, 128, 64), same_geom(layer(BNV, 128, 64, 1.0, 1.0, 1.0f)) }));
    emit("bs opacity above 1", many(TF_BGRA, 2, 128, 64, { layer(BNV, 128, 64), same_geom(layer(BNV, 128, 64, 1.0, 1.0, 1.25f)) }));
    emit("bs opacity NaN", many(TF_BGRA, 2, 128, 64, { layer(BNV, 128, 64), same_geom(layer(BNV, 128, 64, 1.0, 1.0, NAN)) }));
    { Scene s{ TF_BGRA, {}, {} };
      s.tick(128, 64, { layer(BNV, 128, 64), same_geom(layer(BNV, 128, 64)) }).tick(128, 64, { layer(BNV, 128, 64), same_geom(layer(BNV, 128, 64)), same_geom(layer(BNV, 128, 64)) });
      emit("bs mixed n_layers", s); }
    { Scene s = many(TF_BGRA, 2, 128, 64, { layer(BNV, 128, 64), same_geom(layer(BNV, 128, 64)) }); s.t[1].clear_first = 0; emit("bs an uncleared tick", s); }
    { DLayer L = layer(BPL, 128, 64); L.src.pl[2].pitch += 16; emit("bs U/V pitch mismatch", many(TF_BGRA, 2, 128, 64, { L, same_geom(L) })); }
    emit("bs 5 layers", many(TF_BGRA, 2, 128, 64, std::vector<DLayer>(5, same_geom(layer(BNV, 128, 64)))));
    emit("bs flip", many(TF_BGRA, 2, 128, 64, { layer(BNV, 128, 64, 1.0, -1.0), same_geom(layer(BNV, 128, 64, 1.0, -1.0)) }));

    // ---- the tiled kernel ----
    set_switch(&Switches::bgra_path, 2);
    // (main() checks that tile_dims(...).lds of the first IS the budget)
    emit("tiled lds at the budget", many(TF_BGRA, 2, 1024, 32, { layer(BNV, 3296, 166) }));
    emit("tiled lds above the budget", many(TF_BGRA, 2, 1024, 32, { layer(BNV, 3296, 168) }));
    { DLayer L = layer(BNV, 128, 64); L.src.pl[0].ptr = fake(8) + 8; emit("tiled misaligned plane", many(TF_BGRA, 2, 128, 64, { L })); }
    { DLayer L = layer(BNV, 128, 64); L.src.pl[1].pitch += 8; emit("tiled misaligned pitch", many(TF_BGRA, 2, 128, 64, { L })); }
    emit("tiled a plane of fewer than 16 bytes", many(TF_BGRA, 2, 128, 64, { layer(BNV, 12, 64) }));
    { DLayer L = layer(BNV, 128, 64); L.u[U_BORDER + 3] = INFINITY; emit("tiled a matrix entry not finite", many(TF_BGRA, 2, 128, 64, { L })); }
    defaults();
    { Scene s{ TF_BGRA, {}, {} };
      for (int i = 0; i < 63; i++) s.tick(512, 256, { layer(BPL, 512, 256) });
      Scene a = s, b = s;
      a.tick(64, 2032, { layer(BPL, 64, 2032) }); b.tick(64, 2048, { layer(BPL, 64, 2048) });
      emit("tiled y420p 8191 strips", a); emit("tiled y420p 8192 strips", b); }

    // ---- wave_layers_eligible ----
    emit("wave lds at the budget", many(TF_BGRA, 2, 64, 8, { layer(BRGB, 2020, 5, 1.0, 1.0, 0.5f) }));
    emit("wave lds above the budget", many(TF_BGRA, 2, 64, 8, { layer(BRGB, 2024, 5, 1.0, 1.0, 0.5f) }));
    { DLayer L = layer(BRGB, 64, 32); L.src.pl[0].pitch = (1 << 24) - 16; emit("wave pitch below 2^24", many(TF_BGRA, 2, 64, 32, { L }));
      L.src.pl[0].pitch = 1 << 24; emit("wave pitch 2^24", many(TF_BGRA, 2, 64, 32, { L })); }
    { DLayer L = layer(BRGB, 64, 32); L.src.pl[0].h = (1 << 24) - 1; emit("wave height below 2^24", many(TF_BGRA, 2, 64, 32, { L }));
      L.src.pl[0].h = 1 << 24; emit("wave height 2^24", many(TF_BGRA, 2, 64, 32, { L })); }
    emit("wave odd 4:2:0 canvas", many(TF_NV12, 2, 66, 33, { layer(NV, 64, 32) }));
    emit("wave only per-pixel layers", many(TF_BGRA, 2, 128, 64, { rotated(layer(BRGB, 32, 16)) }));
    { Scene s = many(TF_BGRA, 2, 128, 64, { rotated(layer(BRGB, 32, 16)) }); s.t[0].clear_first = s.t[1].clear_first = 0; emit("wave only per-pixel layers, uncleared", s); }
    emit("wave LK_BGRA_METAL among staged layers", many(TF_BGRA, 2, 128, 64, { layer(BNV, 128, 64), layer(LK_BGRA_METAL, 32, 16) }));
    emit("wave LK_BGRA_METAL alone", many(TF_BGRA, 2, 128, 64, { layer(LK_BGRA_METAL, 32, 16) }));
    emit("wave LK_BGRA_METAL on a 4:2:0 canvas", many(TF_NV12, 2, 128, 64, { layer(LK_BGRA_METAL, 32, 16) }));
    emit("wave U/V size mismatch", many(TF_Y420P, 2, 128, 64, { [] { DLayer L = layer(LK_YUV_FROM_Y420P, 128, 64); L.src.pl[2].w = 48; return L; }() }));

    // ---- split batches ----
    for (int videos = 1; videos <= 5; videos++) {
        std::vector<DLayer> ls;
        for (int v = 0; v < videos; v++) ls.push_back(v ? same_geom(layer(BNV, 128, 64, 1.0, 1.0, 0.5f)) : layer(BNV, 128, 64));
        ls.push_back(rotated(layer(BRGB, 32, 16)));
        emit("split " + std::to_string(videos) + " videos + logo", many(TF_BGRA, 2, 128, 64, ls));
    }
    { Scene s{ TF_BGRA, {}, {} };
      std::vector<DLayer> four;
      for (int v = 0; v < 4; v++) four.push_back(v ? same_geom(layer(BNV, 128, 64)) : layer(BNV, 128, 64));
      std::vector<DLayer> five = four; five.push_back(rotated(layer(BRGB, 32, 16)));
      s.tick(128, 64, five).tick(128, 64, four);
      emit("split: every tick keeps one layer", s); }
    { Scene s = many(TF_BGRA, 2, 128, 64, { rotated(layer(BRGB, 32, 16)) }); s.t[0].clear_first = s.t[1].clear_first = 0; emit("tail: uncleared, per-pixel layers only", s);
      set_switch(&Switches::force_general, 1); emit("tail: the same, force_general", s); defaults(); }

    // ---- plan_wave_layers, through wave_geom_config and wave_layers_by_value ----
    emit("plan 8-row strips", many(TF_NV12, 2, 1024, 512, { layer(NV, 1024, 512) }));
    emit("plan 16-row strips", many(TF_NV12, 16, 1024, 512, { layer(NV, 1024, 512) }));
    set_switch(&Switches::wave_rows, 16); emit("plan wave_rows=16", many(TF_NV12, 2, 1024, 512, { layer(NV, 1024, 512) }));
    emit("plan lone bgra tick wave_rows=16", one(TF_BGRA, 128, 64, { layer(BNV, 128, 64) }));
    set_switch(&Switches::wave_rows, 8); emit("plan wave_rows=8", many(TF_NV12, 16, 1024, 512, { layer(NV, 1024, 512) }));
    defaults();
    emit("plan bgra coverage 0.9", many(TF_BGRA, 16, 1000, 512, { layer(BRGB, 1000, 512), with_bbox(layer(BRGB, 500, 256, 1.0, 1.0, 0.5f), 0, 0, 900, 512) }));
    emit("plan bgra coverage below 0.9", many(TF_BGRA, 16, 1000, 512, { layer(BRGB, 1000, 512), with_bbox(layer(BRGB, 500, 256, 1.0, 1.0, 0.5f), 0, 0, 899, 512) }));
    emit("plan 16 rows within LDS_BUDGET / 2", many(TF_BGRA, 16, 1024, 512, { layer(BRGB, 4096, 512) }));
    emit("plan 16 rows beyond LDS_BUDGET / 2", many(TF_BGRA, 16, 1024, 512, { layer(BRGB, 8192, 512) }));
    emit("plan side by side", many(TF_NV12, 2, 256, 64, { layer(NV, 256, 64), layer(RGB, 256, 64, 1.0, 1.0, 0.5f) }));
    emit("plan side by side, planar", many(TF_Y420P, 2, 256, 64, { layer(PL, 256, 64), layer(RGB, 256, 64, 1.0, 1.0, 0.5f) }));
    emit("plan side by side not taken", many(TF_NV12, 2, 256, 64, { layer(NV, 256, 64) }));
    emit("plan shrink", many(TF_BGRA, 2, 64, 8, { layer(BRGB, 2020, 5, 1.0, 1.0, 0.5f), layer(BNV, 64, 16, 1.0, 1.0, 0.5f) }));
    emit("plan lone bgra tick with a per-pixel layer", one(TF_BGRA, 128, 64, { layer(BNV, 128, 64), rotated(layer(BRGB, 32, 16)) }));
    emit("plan lone bgra tick of rgb only", one(TF_BGRA, 128, 64, { layer(BRGB, 128, 64) }));
    { Scene s = one(TF_BGRA, 128, 64, { layer(BNV, 128, 64) }); s.t[0].clear_first = 0; emit("plan lone bgra tick, uncleared", s); }
    emit("plan lone 4:2:0 tick of 7 layers", one(TF_NV12, 64, 32, std::vector<DLayer>(7, layer(NV, 64, 32, 1.0, 1.0, 0.5f))));
    defaults();
}

}  // namespace

#ifndef TICK_ROUTE_DRIVER
namespace {

struct Answer { const char *name, *line; };
const Answer kAnswers[] = {
#include "tick_route_answers.inc"
};
// ys_round for tf = NV12 then y420p, kinds 1 .. 15, 1 .. 4 layers: (kinds << 4) | layers after rounding
const uint8_t kYsRound[2][15][4] = {
#include "tick_route_ys_round.inc"
};

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
                                                                      std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

}  // namespace

int main(int argc, char **) {
    size_t at = 0;
    const size_t n = sizeof kAnswers / sizeof kAnswers[0];
    cases([&](const std::string &name, const Scene &s) {
        const std::string got = answers(s);
        if (argc > 1) { std::printf("{ \"%s\", \"%s\" },\n", name.c_str(), got.c_str()); return; }      // (any argument: print instead of check)
        CHECK(at < n && name == kAnswers[at].name, "case %zu is \"%s\", the table has \"%s\"", at, name.c_str(), at < n ? kAnswers[at].name : "nothing");
        if (at < n) CHECK(got == kAnswers[at].line, "%s:\n  now    %s\n  before %s", name.c_str(), got.c_str(), kAnswers[at].line);
        at++;
    });
    if (argc > 1) return 0;
    CHECK(at == n, "%zu cases, %zu answers", at, n);

    for (int tf = 0; tf < 2; tf++)
        for (int kinds = 1; kinds <= 15; kinds++)
            for (int nl = 1; nl <= 4; nl++) {
                YsPlan p{ kinds, nl, 0 };
                ys_round(tf == 0 ? TF_NV12 : TF_Y420P, p);
                CHECK(((p.kinds << 4) | p.nl) == kYsRound[tf][kinds - 1][nl - 1], "ys_round(%d, kinds %d, %d layers): kinds %d, %d layers, before 0x%02x", tf, kinds, nl,
                      p.kinds, p.nl, kYsRound[tf][kinds - 1][nl - 1]);
            }

    // the bounds the cases above sit on, in the rules' own numbers
    {
        Scene at_budget{ TF_BGRA, {}, {} }, above{ TF_BGRA, {}, {} };
        at_budget.tick(1024, 32, { layer(LK_BGRA_FROM_NV12, 3296, 166) }); above.tick(1024, 32, { layer(LK_BGRA_FROM_NV12, 3296, 168) });
        CHECK(tile_dims(at_budget.t[0], at_budget.l[0], TH_SMALL).lds == (size_t)LDS_BUDGET, "tiled lds at the budget: %zu", tile_dims(at_budget.t[0], at_budget.l[0], TH_SMALL).lds);
        CHECK(tile_dims(above.t[0], above.l[0], TH_SMALL).lds > (size_t)LDS_BUDGET, "tiled lds above the budget: %zu", tile_dims(above.t[0], above.l[0], TH_SMALL).lds);
        Scene w0{ TF_BGRA, {}, {} }, w1{ TF_BGRA, {}, {} };
        w0.tick(64, 8, { layer(LK_BGRA_FROM_RGB, 2020, 5) }); w1.tick(64, 8, { layer(LK_BGRA_FROM_RGB, 2024, 5) });
        CHECK(wave_lds(wave_dims(w0.t[0], w0.l[0], 8), false, TF_BGRA, 8) == (size_t)LDS_BUDGET, "wave lds at the budget: %zu", wave_lds(wave_dims(w0.t[0], w0.l[0], 8), false, TF_BGRA, 8));
        CHECK(wave_lds(wave_dims(w1.t[0], w1.l[0], 8), false, TF_BGRA, 8) > (size_t)LDS_BUDGET, "wave lds above the budget: %zu", wave_lds(wave_dims(w1.t[0], w1.l[0], 8), false, TF_BGRA, 8));
        Scene y3{ TF_NV12, {}, {} }, y4{ TF_NV12, {}, {} };
        y3.tick(64, 32, std::vector<DLayer>(3, layer(LK_YUV_FROM_NV12, 64, 32))); y4.tick(64, 32, std::vector<DLayer>(4, layer(LK_YUV_FROM_NV12, 64, 32)));
        for (Scene *s : { &y3, &y4 }) {
            YsPlan p = ys_plan(s->t.data(), s->l.data(), 1);
            ys_round(TF_NV12, p);
            const int bytes = ys_wave_bytes(p, s->t.data(), s->l.data(), 1);
            CHECK((bytes <= 16 * 1024) == (s == &y3), "tick_yuv_stream wave bytes: %d", bytes);
        }
    }
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
#endif
