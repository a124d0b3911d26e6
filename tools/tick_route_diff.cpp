// tools/tick_route_diff.cpp — do two builds of libchipvideo.so route ticks alike?  Prints what the selection functions (select_fast_path,
// select_tail_path, split_stream_prefix, wave_layers_by_value, the *_eligible predicates, wave_geom_config) answer for the cases of
// tests/cpp/test_tick_route.cpp and for a seeded pseudo-random corpus of launches; run it against each library and compare the outputs
// byte for byte.  The library loads without a GPU.  stderr: how many launches landed on each route.  profiles/tick_route_notes.md has the
// command lines.
//   g++ -std=c++17 -O2 -ffp-contract=off -Iswiftvideo_amd/csrc -Iinclude tools/tick_route_diff.cpp -L<dir of the library> -lchipvideo ...
//   tick_route_diff [launches [seed]]        (first the cases as lines of tests/cpp/tick_route_answers.inc, then one line per launch)
#define TICK_ROUTE_DRIVER
#include "../tests/cpp/test_tick_route.cpp"
#include "chipvideo.h"

static void set_switch(std::atomic<int> Switches::*which, int value) {
    static const char *const bgra[4] = { "", "wave", "tiled", "stream" };
    const std::string v = std::to_string(value);
    if (which == &Switches::bgra_path) chv_debug_set_switch("CHV_BGRA_PATH", bgra[value & 3]);
    else chv_debug_set_switch(which == &Switches::force_general ? "CHV_FORCE_GENERAL" : which == &Switches::wave_rows ? "CHV_WAVE_ROWS" :
                              which == &Switches::stream ? "CHV_STREAM" : "CHV_YUV_STREAM", v.c_str());
}

static uint64_t rng_state;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }
static int pick(int n) { return (int)(rnd() % (uint32_t)n); }
static bool chance(int percent) { return pick(100) < percent; }

int main(int argc, char **argv) {
    const long launches = argc > 1 ? atol(argv[1]) : 240000;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x7153A9D1C0FFEE11ull;
    cases([](const std::string &name, const Scene &s) { std::printf("{ \"%s\", \"%s\" },\n", name.c_str(), answers(s).c_str()); });

    static const int sizes[][2] = { { 8, 4 }, { 64, 32 }, { 128, 64 }, { 200, 120 }, { 640, 360 }, { 992, 504 }, { 1000, 500 }, { 1280, 720 }, { 1400, 1000 }, { 1920, 1080 }, { 3840, 2160 } };
    static const double scales[] = { 0.25, 0.5, 1.0, 1.0, 1.0, 1.5, 1.75, 2.0, 2.125, 3.0, 4.0, 4.5, -1.0 };
    long hist[FP_COUNT + 1] = {};
    for (long i = 0; i < launches; i++) {
        // switches: mostly the defaults, otherwise any combination
        defaults();
        if (chance(40)) {
            set_switch(&Switches::force_general, chance(5)); set_switch(&Switches::bgra_path, pick(4)); set_switch(&Switches::stream, !chance(20));
            set_switch(&Switches::yuv_stream, pick(3)); set_switch(&Switches::wave_rows, chance(30) ? (chance(50) ? 8 : 16) : 0);
        }
        const int tf = chance(50) ? TF_BGRA : chance(50) ? TF_NV12 : TF_Y420P;
        const bool clean = chance(60);                  // nothing odd: the launches that reach the fast routes
        const int n_ticks = chance(45) ? 1 : chance(3) ? 64 + pick(80) : 2 + pick(5);
        const int *sz = sizes[pick(11)];
        int W = sz[0], H = sz[1];
        if (!clean && chance(30)) { W += pick(9) - 4; H += pick(5) - 2; if (W < 1) W = 1; if (H < 1) H = 1; }
        // a tick's layers: a mixer's stack (videos of one geometry, then overlays) or anything
        const int shape = pick(6);                      // 0 nothing / clear, 1 one video, 2 videos of one geometry, 3 videos + overlay, 4 integer RGB frame, 5 anything
        const int own_nv = tf == TF_BGRA ? LK_BGRA_FROM_NV12 : LK_YUV_FROM_NV12, own_pl = tf == TF_BGRA ? LK_BGRA_FROM_Y420P : LK_YUV_FROM_Y420P;
        const int own_rgb = tf == TF_BGRA ? LK_BGRA_FROM_RGB : LK_YUV_FROM_RGB;
        const int video = (tf == TF_Y420P || chance(35)) ? own_pl : own_nv;
        const double kx = clean ? scales[1 + pick(5)] : scales[pick(13)], ky = clean ? scales[1 + pick(5)] : scales[pick(13)];
        const int sw = ((int)(W * (chance(70) ? 1.0 : 1.5)) + 15) & ~15, sh = (H + 1) & ~1;
        std::vector<DLayer> ls;
        auto push_video = [&](bool first) {
            DLayer L = layer(video, sw, sh, kx, ky, first || chance(40) ? 1.f : 0.5f);
            ls.push_back(first ? L : same_geom(L));
        };
        auto push_any = [&] {
            const int kind = chance(70) ? (chance(50) ? video : own_rgb) : pick(8);
            DLayer L = layer(kind, 16 + 4 * pick(200), 2 + 2 * pick(150), scales[pick(13)], scales[pick(13)], chance(50) ? 1.f : 0.25f * (float)pick(6));
            if (chance(25)) L = rotated(L);
            if (chance(10)) L.flags &= ~LF_BOUNDED;
            if (chance(10)) L.flags &= ~LF_NO_FILL;
            if (chance(5)) L.flags |= LF_SAME_GEOM;
            if (chance(8)) { DPlane &P = L.src.pl[pick(3)]; P.ptr = (uint8_t *)((uintptr_t)P.ptr + (1u << pick(4))); }
            if (chance(8)) L.src.pl[pick(3)].pitch += 4 << pick(3);
            if (chance(4)) L.u[pick(48)] = chance(50) ? NAN : INFINITY;
            if (chance(4)) L.u[U_OPACITY] = NAN;
            if (chance(30)) L = with_bbox(L, pick(W), pick(H), W - pick(W / 2 + 1), H - pick(H / 2 + 1));
            L.csc = pick(4);
            ls.push_back(L);
        };
        if (shape == 1) push_video(true);
        else if (shape == 2 || shape == 3) { const int nv = 1 + pick(4); for (int v = 0; v < nv; v++) push_video(v == 0); }
        if (shape == 3) { ls.push_back(chance(50) ? rotated(layer(own_rgb, 320, 180, 0.25, 0.25)) : layer(own_rgb, (W / 2 + 3) & ~3, (H / 2 + 1) & ~1, 1.0, 1.0, 0.5f)); }
        if (shape == 4) ls.push_back(layer(tf == TF_BGRA ? LK_BGRA_FROM_RGB : LK_YUV_FROM_RGB_INT, (W + 3) & ~3, H, 1.0, 1.0));
        if (shape == 5) { const int nl = pick(8); for (int l = 0; l < nl; l++) push_any(); }
        if (!clean && !ls.empty() && chance(50)) push_any();
        for (DLayer &L : ls) if (chance(clean ? 10 : 30)) L.csc = pick(4);
        Scene s{ tf, {}, {} };
        for (int t = 0; t < n_ticks; t++) s.tick(W, H, ls);
        if (!clean || shape == 5) {
            if (chance(25)) for (DTick &T : s.t) T.clear_first = 0;
            if (chance(5)) s.t[(size_t)pick(n_ticks)].clear_first ^= 1;
            if (chance(5)) { DPlane &P = s.t[0].dst.pl[pick(3)]; P.ptr = (uint8_t *)((uintptr_t)P.ptr + (1u << pick(4))); }
            if (chance(5)) s.t[0].dst.pl[pick(3)].pitch += 2 << pick(3);
            if (chance(5) && n_ticks > 1 && s.t[1].n_layers > 0) s.t[1].n_layers--;
        }
        std::printf("%ld tf %d ticks %d: %s\n", i, tf, n_ticks, answers(s).c_str());
        const int route = n_ticks == 1 && chance(50) ? select_fast_path(tf, s.t.data(), s.l.data(), 1, true) : select_fast_path(tf, s.t.data(), s.l.data(), n_ticks);
        hist[route + 1]++;
    }
    for (int p = -1; p < FP_COUNT; p++) std::fprintf(stderr, "%-24s %ld\n", p < 0 ? "FP_NONE" : fast_path_name(p), hist[p + 1]);
    return 0;
}
