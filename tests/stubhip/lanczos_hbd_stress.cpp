// tests/stubhip/lanczos_hbd_stress.cpp — the host path of chv_scale_lanczos_hbd_to_420 / chv_scale_lanczos_hbd_to_420_ladder under sanitizers
// (tests/test_lanczos_hbd_sanitizers.py): chipvideo.cpp for the CPU against the stand-in runtime, whose streams execute LAZILY, and the
// stand-in launcher (stub_lanczos_hbd_launcher.cpp), which reads the ends of every table of every target plane of every rung and touches
// every plane's ends — a source plane's as 16-bit words — when the stream gets to it.  Ladders of 1 .. 8 rungs of both 10-bit sources into
// both targets, lists one picture longer than a chunk, ladders of eight fresh geometries churning the table cache, every refusal (the odd
// start, the odd pitch, 8-bit sources among them), an injected failure of the second of two launches — first on one thread, then on several
// with a context each while two more free and re-create pictures of their own.  No pixels (tests/ -m gpu).
// `lanczos_hbd_stress unregistered`: a build without the launcher unit — the entries answer CHV_ERR_NOT_IMPLEMENTED after validation.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "chipvideo.h"

void stubhip_fail_launch_after(int n);      // stub_runtime.cpp

#define CK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s:%d %s -> %s (%s)\n", __FILE__, __LINE__, #x, chv_error_string(rc_), chv_last_error_detail()); exit(2); } } while (0)
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d expectation failed: %s\n", __FILE__, __LINE__, #cond); exit(3); } } while (0)

static const int kSources[2] = { CHV_FMT_P010, CHV_FMT_Y420P10 };
static const int kTargets[2] = { CHV_FMT_NV12, CHV_FMT_Y420P };
static int planes_of(int fmt) { return fmt == CHV_FMT_NV12 || fmt == CHV_FMT_P010 ? 2 : fmt == CHV_FMT_BGRA ? 1 : 3; }

struct Pic { chv_buffer *buf = nullptr; chv_image img; };
static Pic make_pic(chv_context *c, int fmt, int w, int h) {
    Pic p; memset(&p.img, 0, sizeof p.img);
    p.img.format = fmt; p.img.width = w; p.img.height = h;
    const int cw = w / 2 > 0 ? w / 2 : 1, ch = h / 2 > 0 ? h / 2 : 1;
    const size_t luma = (size_t)w * h, chroma = (size_t)cw * ch;
    if (fmt == CHV_FMT_BGRA) {
        size_t pitch = 0;
        CK(chv_plane_alloc(c, w, h, 4, &p.buf, &pitch));
        p.img.n_planes = 1;
        p.img.planes[0] = chv_plane{ p.buf, 0, w, h, (int32_t)pitch, 4 };
    } else if (fmt == CHV_FMT_NV12) {
        CK(chv_buffer_alloc(c, luma + 2 * chroma, &p.buf));
        p.img.n_planes = 2;
        p.img.planes[0] = chv_plane{ p.buf, 0, w, h, w, 1 };
        p.img.planes[1] = chv_plane{ p.buf, luma, cw, ch, 2 * cw, 2 };
    } else if (fmt == CHV_FMT_Y420P) {
        CK(chv_buffer_alloc(c, luma + 2 * chroma, &p.buf));
        p.img.n_planes = 3;
        p.img.planes[0] = chv_plane{ p.buf, 0, w, h, w, 1 };
        p.img.planes[1] = chv_plane{ p.buf, luma, cw, ch, cw, 1 };
        p.img.planes[2] = chv_plane{ p.buf, luma + chroma, cw, ch, cw, 1 };
    } else if (fmt == CHV_FMT_P010) {
        CK(chv_buffer_alloc(c, 2 * luma + 4 * chroma, &p.buf));
        p.img.n_planes = 2;
        p.img.planes[0] = chv_plane{ p.buf, 0, w, h, 2 * w, 2 };
        p.img.planes[1] = chv_plane{ p.buf, 2 * luma, cw, ch, 4 * cw, 4 };
    } else {
        CK(chv_buffer_alloc(c, 2 * luma + 4 * chroma, &p.buf));
        p.img.n_planes = 3;
        p.img.planes[0] = chv_plane{ p.buf, 0, w, h, 2 * w, 2 };
        p.img.planes[1] = chv_plane{ p.buf, 2 * luma, cw, ch, 2 * cw, 2 };
        p.img.planes[2] = chv_plane{ p.buf, 2 * luma + 2 * chroma, cw, ch, 2 * cw, 2 };
    }
    return p;
}
static uint8_t first_byte(chv_context *c, const Pic &p) {
    uint8_t b = 0;
    CK(chv_download(c, &b, 1, p.buf, 0, (size_t)p.img.planes[0].pitch, 1, 1));
    return b;
}
static unsigned long long launches() {
    unsigned long long v = 0;
    CK(chv_debug_get_counter("lanczos_hbd_launches", &v));
    return v;
}

// rung widths from a 96 x 48 source, heights half of them
static const int kW[8] = { 96, 64, 48, 40, 32, 120, 16, 72 };
static const int kSW = 96, kSH = 48;
static int taps(int in, int out) { const double s = (double)in / out; return 2 * (int)std::ceil(3.0 * (s > 1.0 ? s : 1.0)); }
// the stand-in launcher's rule: the second launch takes the rungs with a logical image beyond 22 taps on an axis
static bool tile_rung(int w, int h) {
    const int dw = w / 2 > 0 ? w / 2 : 1, dh = h / 2 > 0 ? h / 2 : 1;
    return taps(kSW, w) > 22 || taps(kSH, h) > 22 || taps(kSW / 2, dw) > 22 || taps(kSH / 2, dh) > 22;
}

struct Ladder {
    std::vector<Pic> src, dst;                  // dst[r * n + i]
    std::vector<chv_image> ss, ds;
    int n_rungs, n, routes;
};
static Ladder make_ladder(chv_context *c, int sfmt, int dfmt, int n_rungs, int n, int salt = 0) {
    Ladder l; l.n_rungs = n_rungs; l.n = n;
    bool strip = false, tile = false;
    for (int i = 0; i < n; i++) { l.src.push_back(make_pic(c, sfmt, kSW, kSH)); l.ss.push_back(l.src.back().img); }
    for (int r = 0; r < n_rungs; r++) {
        const int w = kW[r] + 2 * salt, h = kW[r] / 2 + salt;
        (tile_rung(w, h) ? tile : strip) = true;
        for (int i = 0; i < n; i++) { l.dst.push_back(make_pic(c, dfmt, w, h)); l.ds.push_back(l.dst.back().img); }
    }
    l.routes = (strip ? 1 : 0) + (tile ? 1 : 0);
    return l;
}
static void free_ladder(Ladder &l) {
    for (Pic &p : l.src) CK(chv_buffer_free(p.buf));
    for (Pic &p : l.dst) CK(chv_buffer_free(p.buf));
}

// a ladder run `times` times; the stamps say every rung of every picture was reached once per run
static void run_ladder(chv_context *c, int sfmt, int dfmt, int n_rungs, int n, int times, bool count) {
    Ladder l = make_ladder(c, sfmt, dfmt, n_rungs, n);
    const unsigned long long before = launches();
    for (int t = 0; t < times; t++) CK(chv_scale_lanczos_hbd_to_420_ladder(c, l.ds.data(), n_rungs, l.ss.data(), n));
    if (count) {
        const int per = CHV_420_LADDER_CHUNK(n_rungs, planes_of(dfmt), planes_of(sfmt)), chunks = (n + per - 1) / per;
        EXPECT(launches() - before == (unsigned long long)times * chunks * l.routes);
    }
    CK(chv_pass_end(c, 1));
    for (const Pic &p : l.dst) EXPECT(first_byte(c, p) == (uint8_t)(0xCD + times));
    free_ladder(l);
}

// eight fresh geometries per call, nobody waits in between: evicted tables are retired while launches that use them are queued, and the
// ladder that comes back last finds its own tables evicted
static void churn(chv_context *c, int sfmt, int dfmt, int salt) {
    std::vector<Ladder> ls;
    for (int k = 0; k < 10; k++) {
        ls.push_back(make_ladder(c, sfmt, dfmt, 8, 2, 1 + k + 10 * (salt % 3)));
        CK(chv_scale_lanczos_hbd_to_420_ladder(c, ls.back().ds.data(), 8, ls.back().ss.data(), 2));
    }
    CK(chv_scale_lanczos_hbd_to_420_ladder(c, ls[0].ds.data(), 8, ls[0].ss.data(), 2));
    CK(chv_pass_end(c, 1));
    for (size_t k = 0; k < ls.size(); k++)
        for (const Pic &p : ls[k].dst) EXPECT(first_byte(c, p) == (uint8_t)(0xCD + (k == 0 ? 2 : 1)));
    for (Ladder &l : ls) free_ladder(l);
}

static void singles(chv_context *c, bool registered) {
    for (int dfmt : kTargets)
        for (int sfmt : kSources) {
            Pic s = make_pic(c, sfmt, kSW, kSH), d = make_pic(c, dfmt, 64, 32);
            const unsigned long long before = launches();
            if (registered) {
                CK(chv_scale_lanczos_hbd_to_420(c, &d.img, &s.img));
                EXPECT(launches() - before == 1u);
            } else {
                EXPECT(chv_scale_lanczos_hbd_to_420(c, &d.img, &s.img) == CHV_ERR_NOT_IMPLEMENTED);
                EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, &d.img, 1, &s.img, 1) == CHV_ERR_NOT_IMPLEMENTED);
            }
            CK(chv_pass_end(c, 1));
            EXPECT(first_byte(c, d) == (uint8_t)(0xCD + (registered ? 1 : 0)));
            CK(chv_buffer_free(s.buf)); CK(chv_buffer_free(d.buf));
        }
}

// what validation refuses, with or without a launcher: statuses only
static void validation(chv_context *c, Ladder &x, Ladder &y) {
    Pic bd = make_pic(c, CHV_FMT_BGRA, 32, 16), bs = make_pic(c, CHV_FMT_BGRA, 96, 48), wide = make_pic(c, CHV_FMT_Y420P10, 100, 48);
    Pic nv = make_pic(c, CHV_FMT_NV12, kSW, kSH), yp = make_pic(c, CHV_FMT_Y420P, kSW, kSH);
    std::vector<chv_image> nine(x.ds.begin(), x.ds.end());
    nine.push_back(x.ds[0]); nine.push_back(x.ds[1]);
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, nine.data(), 9, x.ss.data(), 2) == CHV_ERR_INVALID_VALUE);       // nine rungs
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), -1, x.ss.data(), 2) == CHV_ERR_INVALID_VALUE);
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 2, x.ss.data(), -1) == CHV_ERR_INVALID_VALUE);
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, nullptr, 2, x.ss.data(), 2) == CHV_ERR_INVALID_VALUE);
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 2, nullptr, 2) == CHV_ERR_INVALID_VALUE);
    CK(chv_scale_lanczos_hbd_to_420_ladder(c, nullptr, 0, nullptr, 0));                                            // empty ladders are no-ops
    CK(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 0, x.ss.data(), 2));
    CK(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 2, x.ss.data(), 0));
    std::vector<chv_image> mix = { x.ds[0], x.ds[1], y.ds[2], y.ds[3] };                                           // two target formats
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, mix.data(), 2, x.ss.data(), 2) == CHV_ERR_INVALID_VALUE);
    chv_image s2[2] = { x.ss[0], y.ss[1] };                                                                        // a p010 source among y420p10 sources
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 2, s2, 2) == CHV_ERR_INVALID_VALUE);
    std::vector<chv_image> sizes = { x.ds[0], x.ds[1], x.ds[2], x.ds[4] };                                         // two sizes inside a rung
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, sizes.data(), 2, x.ss.data(), 2) == CHV_ERR_INVALID_VALUE);
    chv_image s3[2] = { x.ss[0], wide.img };                                                                       // two source sizes
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 2, s3, 2) == CHV_ERR_INVALID_VALUE);
    std::vector<chv_image> bad(x.ds.begin(), x.ds.begin() + 4);                                                    // a bad chroma plane in the last rung
    bad[3].planes[2].pitch = 3;
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, bad.data(), 2, x.ss.data(), 2) == CHV_ERR_BAD_TARGET);
    bad[3] = x.ds[3]; bad[3].planes[2].width -= 1;                                                                 // a y420p target with unequal chroma planes
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, bad.data(), 2, x.ss.data(), 2) == CHV_ERR_BAD_TARGET);
    EXPECT(chv_scale_lanczos_hbd_to_420(c, &bad[3], &x.ss[0]) == CHV_ERR_BAD_TARGET);
    EXPECT(chv_scale_lanczos_hbd_to_420(c, &bd.img, &x.ss[0]) == CHV_ERR_BAD_TARGET);                              // a BGRA target
    EXPECT(chv_scale_lanczos_hbd_to_420(c, nullptr, &x.ss[0]) == CHV_ERR_BAD_TARGET);
    for (Pic *eight : { &bs, &nv, &yp }) {                                                                         // 8-bit sources are not forwarded
        EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 1, &eight->img, 1) == CHV_ERR_BAD_INPUT);
        EXPECT(chv_scale_lanczos_hbd_to_420(c, &x.ds[0], &eight->img) == CHV_ERR_BAD_INPUT);
    }
    EXPECT(chv_scale_lanczos_hbd_to_420(c, &x.ds[0], nullptr) == CHV_ERR_BAD_INPUT);
    chv_image uneq = x.ss[0]; uneq.planes[1].height -= 1;                                                          // Cb and Cr of different size
    EXPECT(chv_scale_lanczos_hbd_to_420(c, &x.ds[0], &uneq) == CHV_ERR_BAD_INPUT);
    chv_image two_planes = x.ss[0]; two_planes.n_planes = 2;                                                       // y420p10 with two planes
    EXPECT(chv_scale_lanczos_hbd_to_420(c, &x.ds[0], &two_planes) == CHV_ERR_BAD_INPUT);
    chv_image one_comp = y.ss[0]; one_comp.planes[0].components = 1;                                               // a 16-bit plane described with one byte per texel
    EXPECT(chv_scale_lanczos_hbd_to_420(c, &y.ds[0], &one_comp) == CHV_ERR_BAD_INPUT);
    chv_image two_comp = y.ss[0]; two_comp.planes[1].components = 2;                                               // p010's CbCr described as one word per texel
    EXPECT(chv_scale_lanczos_hbd_to_420(c, &y.ds[0], &two_comp) == CHV_ERR_BAD_INPUT);
    chv_image far = y.ss[0]; far.planes[0].offset += (size_t)1 << 30;
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, y.ds.data(), 1, &far, 1) == CHV_ERR_BAD_INPUT);
    for (int p = 0; p < 3; p++) {                                                                                  // an odd start, an odd pitch: every plane
        chv_image odd = x.ss[1]; odd.planes[p].offset += 1; odd.planes[p].height -= 1;
        chv_image two[2] = { x.ss[0], odd };
        EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 1, two, 2) == CHV_ERR_BAD_INPUT);
        odd = x.ss[1]; odd.planes[p].pitch += 1; odd.planes[p].height = 1;
        two[1] = odd;
        EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 1, two, 2) == CHV_ERR_BAD_INPUT);
    }
    for (int p = 0; p < 2; p++) {
        chv_image odd = y.ss[0]; odd.planes[p].offset += 1; odd.planes[p].height -= 1;
        EXPECT(chv_scale_lanczos_hbd_to_420(c, &y.ds[0], &odd) == CHV_ERR_BAD_INPUT);
    }
    // the existing entries refuse the two new formats as they refuse any unknown format
    EXPECT(chv_scale_lanczos(c, &x.ds[0], &x.ss[0]) == CHV_ERR_BAD_INPUT);
    EXPECT(chv_scale_lanczos_420(c, &x.ds[0], &x.ss[0]) == CHV_ERR_BAD_INPUT);
    EXPECT(chv_scale_lanczos_to_420(c, &y.ds[0], &y.ss[0]) == CHV_ERR_BAD_INPUT);
    EXPECT(chv_scale_lanczos_to_420_ladder(c, y.ds.data(), 1, y.ss.data(), 1) == CHV_ERR_BAD_INPUT);
    for (Pic *p : { &bd, &bs, &wide, &nv, &yp }) CK(chv_buffer_free(p->buf));
}

static void refusals(chv_context *c) {
    Ladder x = make_ladder(c, CHV_FMT_Y420P10, CHV_FMT_Y420P, 8, 2), y = make_ladder(c, CHV_FMT_P010, CHV_FMT_NV12, 2, 2);
    const unsigned long long before = launches();
    validation(c, x, y);
    // the 160 KB rule in the LAST rung: nothing is launched for the first
    Pic big = make_pic(c, CHV_FMT_P010, 640, 64), first = make_pic(c, CHV_FMT_NV12, 64, 32), tiny = make_pic(c, CHV_FMT_NV12, 16, 8);
    chv_image two[2] = { first.img, tiny.img };
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, two, 2, &big.img, 1) == CHV_ERR_INVALID_VALUE);
    EXPECT(chv_scale_lanczos_hbd_to_420(c, &tiny.img, &big.img) == CHV_ERR_INVALID_VALUE);
    EXPECT(launches() == before);
    CK(chv_scale_lanczos_hbd_to_420(c, &first.img, &big.img));
    EXPECT(launches() == before + 1);
    // the second of two launches fails: an error, one launch counted; the next call works
    EXPECT(x.routes == 2);
    stubhip_fail_launch_after(2);
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 8, x.ss.data(), 2) != CHV_OK);
    EXPECT(launches() == before + 2);
    stubhip_fail_launch_after(1);
    EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 8, x.ss.data(), 2) != CHV_OK);
    EXPECT(launches() == before + 2);
    CK(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 8, x.ss.data(), 2));
    EXPECT(launches() == before + 4);
    CK(chv_pass_end(c, 1));
    for (int r = 0; r < 8; r++)
        for (int i = 0; i < 2; i++)      // (the first launch of the failed call: the rungs of at most 22 taps)
            EXPECT(first_byte(c, x.dst[(size_t)r * 2 + i]) == (uint8_t)(0xCD + (tile_rung(kW[r], kW[r] / 2) ? 1 : 2)));
    for (const Pic &p : y.dst) EXPECT(first_byte(c, p) == 0xCD);
    EXPECT(first_byte(c, first) == 0xCD + 1 && first_byte(c, tiny) == 0xCD);
    free_ladder(x); free_ladder(y);
    for (Pic *p : { &big, &first, &tiny }) CK(chv_buffer_free(p->buf));
}

// the ladder inside a pass: held work is flushed in front of it, and the pass goes on
static void inside_a_pass(chv_context *c) {
    Ladder l = make_ladder(c, CHV_FMT_P010, CHV_FMT_Y420P, 3, 1);
    Pic canvas = make_pic(c, CHV_FMT_NV12, 64, 32);
    CK(chv_pass_begin(c));
    CK(chv_run_kernel(c, CHV_K_IMG_CLEAR_NV12, &canvas.img, nullptr, 0, nullptr, 0, 0, nullptr));
    CK(chv_scale_lanczos_hbd_to_420_ladder(c, l.ds.data(), 3, l.ss.data(), 1));
    CK(chv_scale_lanczos_hbd_to_420(c, &l.ds[0], &l.ss[0]));
    CK(chv_pass_end(c, 1));
    for (size_t k = 0; k < l.dst.size(); k++) EXPECT(first_byte(c, l.dst[k]) == (uint8_t)(0xCD + (k == 0 ? 2 : 1)));
    free_ladder(l);
    CK(chv_buffer_free(canvas.buf));
}

static void worker(int device, int id) {
    chv_context *c = nullptr;
    CK(chv_context_create(device, &c));
    const int sfmt = kSources[id % 2], dfmt = kTargets[(id / 2) % 2];
    for (int rep = 0; rep < 3; rep++) {
        const int n_rungs = 1 + (id + rep) % 8;
        run_ladder(c, sfmt, dfmt, n_rungs, CHV_420_LADDER_CHUNK(n_rungs, planes_of(dfmt), planes_of(sfmt)) + 1, 2, false);
        churn(c, sfmt, dfmt, id + rep);
    }
    CK(chv_context_destroy(c));
}

// pictures of its own, made, converted once and freed without a wait of its own (chv_buffer_free waits for the device), while the workers run
static void recreator(int device, std::atomic<bool> *stop) {
    chv_context *c = nullptr;
    CK(chv_context_create(device, &c));
    for (int r = 0; !stop->load() || r < 20; r++) {
        Ladder l = make_ladder(c, kSources[r % 2], kTargets[(r / 2) % 2], 1 + r % 8, 1 + r % 2, r % 5);
        CK(chv_scale_lanczos_hbd_to_420_ladder(c, l.ds.data(), l.n_rungs, l.ss.data(), l.n));
        free_ladder(l);
        if (r > 4000) break;
    }
    CK(chv_context_destroy(c));
}

int main(int argc, char **argv) {
    chv_context *c = nullptr;
    CK(chv_context_create(0, &c));
    if (argc > 1 && !strcmp(argv[1], "unregistered")) {
        Ladder x = make_ladder(c, CHV_FMT_Y420P10, CHV_FMT_Y420P, 8, 2), y = make_ladder(c, CHV_FMT_P010, CHV_FMT_NV12, 3, 2);
        EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, x.ds.data(), 3, x.ss.data(), 2) == CHV_ERR_NOT_IMPLEMENTED);
        EXPECT(chv_scale_lanczos_hbd_to_420_ladder(c, y.ds.data(), 3, y.ss.data(), 2) == CHV_ERR_NOT_IMPLEMENTED);
        validation(c, x, y);                                                                                       // (validation comes first)
        CK(chv_pass_end(c, 1));
        for (const Pic &p : x.dst) EXPECT(first_byte(c, p) == 0xCD);
        singles(c, false);
        EXPECT(launches() == 0);
        free_ladder(x); free_ladder(y);
        CK(chv_context_destroy(c));
        printf("lanczos_hbd_stress: not implemented without a launcher, ok\n");
        return 0;
    }
    const int threads = argc > 1 ? atoi(argv[1]) : 6;
    for (int sfmt : kSources) {
        for (int dfmt : kTargets) {
            const int dp = planes_of(dfmt), sp = planes_of(sfmt);
            for (int n_rungs = 1; n_rungs <= 8; n_rungs++) run_ladder(c, sfmt, dfmt, n_rungs, 3, 2, true);
            run_ladder(c, sfmt, dfmt, 1, CHV_420_LADDER_CHUNK(1, dp, sp) + 1, 2, true);          // one more than a chunk
            run_ladder(c, sfmt, dfmt, 3, 2 * CHV_420_LADDER_CHUNK(3, dp, sp) + 1, 1, true);       // three chunks
            run_ladder(c, sfmt, dfmt, 8, CHV_420_LADDER_CHUNK(8, dp, sp) + 1, 2, true);          // two launches in each of two chunks
        }
        churn(c, sfmt, kTargets[sfmt & 1], 0);
    }
    singles(c, true);
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
    printf("lanczos_hbd_stress: ok\n");
    return 0;
}
