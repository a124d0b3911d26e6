// tests/stubhip/lanczos_rgb_ladder_stress.cpp — the host path of chv_scale_lanczos_rgb_ladder under sanitizers
// (tests/test_lanczos_rgb_ladder_sanitizers.py): chipvideo.cpp for the CPU against the stand-in runtime, whose streams execute LAZILY, and the
// stand-in launcher (stub_lanczos_rgb_ladder_launcher.cpp), which reads the ends of both tables of every rung and touches every plane's ends
// when the stream gets to it.  Ladders of one to eight rungs in both byte orders, lists one picture longer than a chunk and of three chunks,
// fresh geometries churning the table cache while 16 references are held, every refusal, an injected launch failure on the second of two
// launches — first on one thread, then on several with a context each while two more free and re-create pictures of their own.  No pixels
// (tests/ -m gpu).
// `lanczos_rgb_ladder_stress unregistered`: a build without a launcher unit — the entry answers CHV_ERR_NOT_IMPLEMENTED after validation.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "chipvideo.h"

void stubhip_fail_launch_after(int n);      // stub_runtime.cpp

#define CK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s:%d %s -> %s (%s)\n", __FILE__, __LINE__, #x, chv_error_string(rc_), chv_last_error_detail()); exit(2); } } while (0)
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d expectation failed: %s\n", __FILE__, __LINE__, #cond); exit(3); } } while (0)

static_assert(CHV_RGB_LADDER_CHUNK(1) == 124 && CHV_RGB_LADDER_CHUNK(8) == 27, "include/chipvideo.h states the rule");

struct Pic { chv_buffer *buf = nullptr; chv_image img; };
static Pic make_pic(chv_context *c, int fmt, int w, int h) {
    Pic p; memset(&p.img, 0, sizeof p.img);
    p.img.format = fmt; p.img.width = w; p.img.height = h;
    const int cw = w / 2 > 0 ? w / 2 : 1, ch = h / 2 > 0 ? h / 2 : 1;
    if (fmt == CHV_FMT_NV12) {
        CK(chv_buffer_alloc(c, (size_t)w * h + (size_t)2 * cw * ch, &p.buf));
        p.img.n_planes = 2;
        p.img.planes[0] = chv_plane{ p.buf, 0, w, h, w, 1 };
        p.img.planes[1] = chv_plane{ p.buf, (size_t)w * h, cw, ch, 2 * cw, 2 };
    } else {
        size_t pitch = 0;
        CK(chv_plane_alloc(c, w, h, 4, &p.buf, &pitch));
        p.img.n_planes = 1;
        p.img.planes[0] = chv_plane{ p.buf, 0, w, h, (int32_t)pitch, 4 };
    }
    return p;
}
static uint8_t first_byte(chv_context *c, const Pic &p) {
    uint8_t b = 0;
    CK(chv_download(c, &b, 1, p.buf, 0, (size_t)p.img.planes[0].pitch, 1, 1));
    return b;
}
static unsigned long long counter(const char *name) {
    unsigned long long v = 0;
    CK(chv_debug_get_counter(name, &v));
    return v;
}
static unsigned long long launches() { return counter("lanczos_rgb_ladder_launches"); }
static unsigned long long other_launches() {
    return counter("lanczos_ladder_launches") + counter("lanczos_planar_ladder_launches") + counter("lanczos_420_ladder_launches") +
           counter("lanczos_from_yuv_launches") + counter("lanczos_from_yuv_ladder_launches");
}

// rung sizes from a 96 x 48 (+ salt) source: the first six take the strip route (one of them with 16 and 10 taps), the last two (30 and 48
// taps) the tile route: the stand-in's second launch
static const int kSizes[8][2] = { { 64, 32 }, { 48, 24 }, { 96, 48 }, { 120, 60 }, { 64, 32 }, { 40, 32 }, { 20, 10 }, { 12, 6 } };

struct Ladder {
    std::vector<Pic> src, dst;      // dst[r * n + i]
    std::vector<chv_image> ss, ds;
    int n, n_rungs;
};
// n pictures of 96 x 48 (+ salt); rung r's targets are kSizes[(first + r) % 8] (+ grow)
static Ladder make_ladder(chv_context *c, int fmt, int n, int n_rungs, int first = 0, int salt = 0, int grow = 0) {
    Ladder l; l.n = n; l.n_rungs = n_rungs;
    for (int i = 0; i < n; i++) { l.src.push_back(make_pic(c, fmt, 96 + 2 * salt, 48 + 2 * salt)); l.ss.push_back(l.src.back().img); }
    for (int r = 0; r < n_rungs; r++)
        for (int i = 0; i < n; i++) {
            l.dst.push_back(make_pic(c, fmt, kSizes[(first + r) % 8][0] + grow, kSizes[(first + r) % 8][1] + grow));
            l.ds.push_back(l.dst.back().img);
        }
    return l;
}
static void free_ladder(Ladder &l) {
    for (Pic &p : l.src) CK(chv_buffer_free(p.buf));
    for (Pic &p : l.dst) CK(chv_buffer_free(p.buf));
}
// the routes the rungs [first, first + n_rungs) of kSizes take: 1 or 2 launches per chunk
static int routes(int first, int n_rungs) {
    bool strip = false, tile = false;
    for (int r = 0; r < n_rungs; r++) ((first + r) % 8 >= 6 ? tile : strip) = true;
    return (strip ? 1 : 0) + (tile ? 1 : 0);
}

// a ladder run `times` times; the stamps say every target of every rung was reached once per run
static void run_ladder(chv_context *c, int fmt, int n, int n_rungs, int first, int times, bool count) {
    Ladder l = make_ladder(c, fmt, n, n_rungs, first);
    const unsigned long long before = launches(), others = other_launches();
    for (int t = 0; t < times; t++) CK(chv_scale_lanczos_rgb_ladder(c, l.ds.data(), n_rungs, l.ss.data(), n));
    const int chunk = CHV_RGB_LADDER_CHUNK(n_rungs);
    if (count) {
        EXPECT(launches() - before == (unsigned long long)times * ((n + chunk - 1) / chunk) * routes(first, n_rungs));
        EXPECT(other_launches() == others);
    }
    CK(chv_pass_end(c, 1));
    for (const Pic &p : l.dst) EXPECT(first_byte(c, p) == (uint8_t)(0xCD + times));
    free_ladder(l);
}

// a fresh geometry per rung per call (two tables each, 16 references held per call), nobody waits in between: evicted tables are retired
// while launches that use them are queued, and the ladder that comes back last finds its own tables evicted
static void churn(chv_context *c, int salt) {
    std::vector<Ladder> ls;
    for (int k = 0; k < 12; k++) {
        ls.push_back(make_ladder(c, k & 1 ? CHV_FMT_RGBA : CHV_FMT_BGRA, 2, 8, k, k % 7, k + 13 * (salt % 3)));
        CK(chv_scale_lanczos_rgb_ladder(c, ls.back().ds.data(), 8, ls.back().ss.data(), 2));
    }
    CK(chv_scale_lanczos_rgb_ladder(c, ls[0].ds.data(), 8, ls[0].ss.data(), 2));
    CK(chv_pass_end(c, 1));
    for (size_t k = 0; k < ls.size(); k++)
        for (const Pic &p : ls[k].dst) EXPECT(first_byte(c, p) == (uint8_t)(0xCD + (k == 0 ? 2 : 1)));
    for (Ladder &l : ls) free_ladder(l);
}

static void refusals(chv_context *c) {
    Ladder x = make_ladder(c, CHV_FMT_BGRA, 2, 3), y = make_ladder(c, CHV_FMT_RGBA, 2, 3);
    Pic wide = make_pic(c, CHV_FMT_BGRA, 100, 48), nv = make_pic(c, CHV_FMT_NV12, 96, 48), nvt = make_pic(c, CHV_FMT_NV12, 96, 48);
    const unsigned long long before = launches();
    auto call = [&](const std::vector<chv_image> &ds, int n_rungs, const std::vector<chv_image> &ss, int n) {
        return chv_scale_lanczos_rgb_ladder(c, ds.data(), n_rungs, ss.data(), n);
    };
    // counts and lists
    CK(chv_scale_lanczos_rgb_ladder(c, nullptr, 0, nullptr, 0));
    CK(call(x.ds, 0, x.ss, 2));
    CK(call(x.ds, 3, x.ss, 0));
    EXPECT(call(x.ds, -1, x.ss, 2) == CHV_ERR_INVALID_VALUE);
    EXPECT(call(x.ds, CHV_LADDER_MAX_RUNGS + 1, x.ss, 2) == CHV_ERR_INVALID_VALUE);
    EXPECT(call(x.ds, 3, x.ss, -1) == CHV_ERR_INVALID_VALUE);
    EXPECT(chv_scale_lanczos_rgb_ladder(c, nullptr, 3, x.ss.data(), 2) == CHV_ERR_INVALID_VALUE);
    EXPECT(chv_scale_lanczos_rgb_ladder(c, x.ds.data(), 3, nullptr, 2) == CHV_ERR_INVALID_VALUE);
    // one source size, one size per rung — in the LAST place of each list
    std::vector<chv_image> d = x.ds; d[5] = x.ds[1];                                                           // rung 2 with two sizes
    EXPECT(call(d, 3, x.ss, 2) == CHV_ERR_INVALID_VALUE);
    std::vector<chv_image> s = x.ss; s[1] = wide.img;                                                          // two source sizes
    EXPECT(call(x.ds, 3, s, 2) == CHV_ERR_INVALID_VALUE);
    // a target, a source that is not exactly one plane of 4 components, or whose plane fails a check
    d = x.ds; d[5] = nvt.img;                                                                                  // a 4:2:0 target
    EXPECT(call(d, 3, x.ss, 2) == CHV_ERR_BAD_TARGET);
    d = x.ds; d[5].planes[0].height = 1 << 20;
    EXPECT(call(d, 3, x.ss, 2) == CHV_ERR_BAD_TARGET);
    d = x.ds; d[5].n_planes = 2;
    EXPECT(call(d, 3, x.ss, 2) == CHV_ERR_BAD_TARGET);
    d = x.ds; d[4].planes[0].pitch = 3;
    EXPECT(call(d, 3, x.ss, 2) == CHV_ERR_BAD_TARGET);
    d = x.ds; d[5].planes[0].components = 1;
    EXPECT(call(d, 3, x.ss, 2) == CHV_ERR_BAD_TARGET);
    d = x.ds; d[5].planes[0].buffer = nullptr;
    EXPECT(call(d, 3, x.ss, 2) == CHV_ERR_BAD_TARGET);
    s = x.ss; s[1] = nv.img;                                                                                   // a 4:2:0 source
    EXPECT(call(x.ds, 3, s, 2) == CHV_ERR_BAD_INPUT);
    s = x.ss; s[1].planes[0].components = 2;
    EXPECT(call(x.ds, 3, s, 2) == CHV_ERR_BAD_INPUT);
    s = x.ss; s[1].planes[0].offset += (size_t)1 << 30;
    EXPECT(call(x.ds, 3, s, 2) == CHV_ERR_BAD_INPUT);
    s = x.ss; s[1].planes[0].offset += 2;
    EXPECT(call(x.ds, 3, s, 2) == CHV_ERR_BAD_INPUT);
    // the `format` field of a 4-component image is not read: a ladder of both byte orders is a good ladder (run below)
    // a refused LAST rung after valid ones: 24:1, which the 160 KB rule refuses; more than 256 taps
    Pic big[2] = { make_pic(c, CHV_FMT_BGRA, 96, 96), make_pic(c, CHV_FMT_BGRA, 96, 96) };
    Pic mid[2] = { make_pic(c, CHV_FMT_BGRA, 64, 64), make_pic(c, CHV_FMT_BGRA, 64, 64) }, tiny[2] = { make_pic(c, CHV_FMT_BGRA, 4, 4), make_pic(c, CHV_FMT_BGRA, 4, 4) };
    std::vector<chv_image> bs2 = { big[0].img, big[1].img }, dd = { mid[0].img, mid[1].img, tiny[0].img, tiny[1].img };
    EXPECT(call(dd, 2, bs2, 2) == CHV_ERR_INVALID_VALUE);
    Pic tall[2] = { make_pic(c, CHV_FMT_BGRA, 8, 90), make_pic(c, CHV_FMT_BGRA, 8, 90) }, thin[2] = { make_pic(c, CHV_FMT_BGRA, 8, 2), make_pic(c, CHV_FMT_BGRA, 8, 2) };
    std::vector<chv_image> ts = { tall[0].img, tall[1].img }, td = { tall[0].img, tall[1].img, thin[0].img, thin[1].img };
    EXPECT(call(td, 2, ts, 2) == CHV_ERR_INVALID_VALUE);                                                       // 45:1: 270 taps
    EXPECT(launches() == before);
    // an injected launch failure on the first launch: an error, nothing counted, nothing written
    stubhip_fail_launch_after(1);
    EXPECT(call(x.ds, 3, x.ss, 2) != CHV_OK);
    EXPECT(launches() == before);
    CK(chv_pass_end(c, 1));
    for (const Pic &p : x.dst) EXPECT(first_byte(c, p) == 0xCD);
    for (const Pic &p : y.dst) EXPECT(first_byte(c, p) == 0xCD);
    for (int i = 0; i < 2; i++) EXPECT(first_byte(c, mid[i]) == 0xCD && first_byte(c, tiny[i]) == 0xCD && first_byte(c, thin[i]) == 0xCD && first_byte(c, tall[i]) == 0xCD);
    d = x.ds; d[4] = y.ds[4]; d[5] = y.ds[5];                                                                  // (both byte orders in one ladder)
    CK(call(d, 3, x.ss, 2));
    EXPECT(launches() == before + 1);
    CK(chv_pass_end(c, 1));
    for (int k = 0; k < 4; k++) EXPECT(first_byte(c, x.dst[k]) == (uint8_t)(0xCD + 1));
    EXPECT(first_byte(c, y.dst[4]) == (uint8_t)(0xCD + 1) && first_byte(c, y.dst[5]) == (uint8_t)(0xCD + 1) && first_byte(c, x.dst[4]) == 0xCD);
    // the second of two launches fails (the rungs of the other route): the first was launched and counted
    Ladder z = make_ladder(c, CHV_FMT_BGRA, 2, 3, 5);                                                          // rungs 5 (strip), 6 and 7 (tile)
    stubhip_fail_launch_after(2);
    EXPECT(call(z.ds, 3, z.ss, 2) != CHV_OK);
    EXPECT(launches() == before + 2);
    CK(chv_pass_end(c, 1));
    EXPECT(first_byte(c, z.dst[0]) == (uint8_t)(0xCD + 1) && first_byte(c, z.dst[1]) == (uint8_t)(0xCD + 1));
    for (int k = 2; k < 6; k++) EXPECT(first_byte(c, z.dst[k]) == 0xCD);
    // the second chunk's launch fails: the first chunk was launched and counted
    const int chunk = CHV_RGB_LADDER_CHUNK(2);
    Ladder w = make_ladder(c, CHV_FMT_RGBA, chunk + 1, 2);
    stubhip_fail_launch_after(2);
    EXPECT(call(w.ds, 2, w.ss, w.n) != CHV_OK);
    EXPECT(launches() == before + 3);
    CK(chv_pass_end(c, 1));
    EXPECT(first_byte(c, w.dst[0]) == (uint8_t)(0xCD + 1) && first_byte(c, w.dst[chunk]) == 0xCD);
    EXPECT(first_byte(c, w.dst[w.n + chunk - 1]) == (uint8_t)(0xCD + 1) && first_byte(c, w.dst[w.n + chunk]) == 0xCD);
    free_ladder(x); free_ladder(y); free_ladder(z); free_ladder(w);
    for (Pic *p : { &wide, &nv, &nvt, &big[0], &big[1], &mid[0], &mid[1], &tiny[0], &tiny[1], &tall[0], &tall[1], &thin[0], &thin[1] }) CK(chv_buffer_free(p->buf));
}

// the call inside a pass: held work is flushed in front of it, and the pass goes on
static void inside_a_pass(chv_context *c) {
    Ladder l = make_ladder(c, CHV_FMT_BGRA, 2, 4, 4);
    CK(chv_pass_begin(c));
    CK(chv_run_kernel(c, CHV_K_IMG_CLEAR_BGRA, &l.ss[0], nullptr, 0, nullptr, 0, 0, nullptr));
    CK(chv_scale_lanczos_rgb_ladder(c, l.ds.data(), 4, l.ss.data(), 2));
    CK(chv_scale_lanczos_rgb_ladder(c, l.ds.data(), 1, l.ss.data(), 2));
    CK(chv_pass_end(c, 1));
    for (size_t k = 0; k < l.dst.size(); k++) EXPECT(first_byte(c, l.dst[k]) == (uint8_t)(0xCD + (k < 2 ? 2 : 1)));
    free_ladder(l);
}

static void worker(int device, int id) {
    chv_context *c = nullptr;
    CK(chv_context_create(device, &c));
    const int fmt = id & 1 ? CHV_FMT_RGBA : CHV_FMT_BGRA;
    for (int rep = 0; rep < 3; rep++) {
        const int n_rungs = 1 + (id + 3 * rep) % 8;
        run_ladder(c, fmt, CHV_RGB_LADDER_CHUNK(n_rungs) + 1 + rep, n_rungs, id + rep, 2, false);
        churn(c, id + rep);
    }
    CK(chv_context_destroy(c));
}

// pictures of its own, made, resized once and freed without a wait of its own (chv_buffer_free waits for the device), while the workers run
static void recreator(int device, std::atomic<bool> *stop) {
    chv_context *c = nullptr;
    CK(chv_context_create(device, &c));
    for (int r = 0; !stop->load() || r < 20; r++) {
        Ladder l = make_ladder(c, r % 3 ? CHV_FMT_BGRA : CHV_FMT_RGBA, 1 + r % 3, 1 + r % 8, r, r % 5, r % 50);
        CK(chv_scale_lanczos_rgb_ladder(c, l.ds.data(), l.n_rungs, l.ss.data(), l.n));
        free_ladder(l);
        if (r > 4000) break;
    }
    CK(chv_context_destroy(c));
}

int main(int argc, char **argv) {
    chv_context *c = nullptr;
    CK(chv_context_create(0, &c));
    if (argc > 1 && !strcmp(argv[1], "unregistered")) {
        Ladder x = make_ladder(c, CHV_FMT_BGRA, 2, 3), y = make_ladder(c, CHV_FMT_RGBA, 2, 3);
        Pic nv = make_pic(c, CHV_FMT_NV12, 96, 48);
        EXPECT(chv_scale_lanczos_rgb_ladder(c, x.ds.data(), 3, x.ss.data(), 2) == CHV_ERR_NOT_IMPLEMENTED);
        EXPECT(chv_scale_lanczos_rgb_ladder(c, y.ds.data(), 1, y.ss.data(), 1) == CHV_ERR_NOT_IMPLEMENTED);
        std::vector<chv_image> bad = { x.ds[0], nv.img };
        EXPECT(chv_scale_lanczos_rgb_ladder(c, bad.data(), 1, x.ss.data(), 2) == CHV_ERR_BAD_TARGET);          // (validation comes first)
        bad = { x.ss[0], nv.img };
        EXPECT(chv_scale_lanczos_rgb_ladder(c, x.ds.data(), 1, bad.data(), 2) == CHV_ERR_BAD_INPUT);
        std::vector<chv_image> d2 = x.ds; d2[5] = x.ds[0];
        EXPECT(chv_scale_lanczos_rgb_ladder(c, d2.data(), 3, x.ss.data(), 2) == CHV_ERR_INVALID_VALUE);
        CK(chv_scale_lanczos_rgb_ladder(c, x.ds.data(), 0, x.ss.data(), 2));
        CK(chv_pass_end(c, 1));
        for (const Pic &p : x.dst) EXPECT(first_byte(c, p) == 0xCD);
        EXPECT(launches() == 0);
        free_ladder(x); free_ladder(y);
        CK(chv_buffer_free(nv.buf));
        CK(chv_context_destroy(c));
        printf("lanczos_rgb_ladder_stress: not implemented without a launcher, ok\n");
        return 0;
    }
    const int threads = argc > 1 ? atoi(argv[1]) : 6;
    for (int fmt : { CHV_FMT_BGRA, CHV_FMT_RGBA }) {
        run_ladder(c, fmt, 1, 1, 0, 2, true);
        run_ladder(c, fmt, 3, 4, 4, 2, true);                                                                  // both routes
        run_ladder(c, fmt, 2, 2, 6, 1, true);                                                                  // the tile route alone
        const int chunk8 = CHV_RGB_LADDER_CHUNK(8), chunk1 = CHV_RGB_LADDER_CHUNK(1);
        run_ladder(c, fmt, chunk8, 8, 0, 1, true);                                                             // exactly a chunk
        run_ladder(c, fmt, chunk8 + 1, 8, 0, 2, true);                                                         // one more than a chunk
        run_ladder(c, fmt, 2 * chunk1 + 1, 1, 1, 1, true);                                                     // three chunks
        churn(c, fmt);
    }
    refusals(c);
    inside_a_pass(c);
    std::atomic<bool> stop{false};
    std::thread rec0(recreator, 0, &stop), rec1(recreator, 1, &stop);
    std::vector<std::thread> pool;
    for (int i = 0; i < threads; i++) pool.emplace_back(worker, i % 2, i);
    for (auto &t : pool) t.join();
    stop.store(true);
    rec0.join(); rec1.join();
    CK(chv_context_destroy(c));
    printf("lanczos_rgb_ladder_stress: ok\n");
    return 0;
}
