// tests/stubhip/lanczos_from_yuv_stress.cpp — the host path of chv_scale_lanczos_from_yuv / chv_scale_lanczos_from_yuv_batch under sanitizers
// (tests/test_lanczos_from_yuv_sanitizers.py): chipvideo.cpp for the CPU against the stand-in runtime, whose streams execute LAZILY, and the
// stand-in launcher (stub_lanczos_from_yuv_launcher.cpp), which reads the ends of all four tables and touches every plane's ends when the
// stream gets to it.  Single calls and lists of both packings into both target orders, lists one picture longer than a chunk and of three
// chunks, fresh geometries churning the table cache, every refusal, an injected launch failure — first on one thread, then on several with a
// context each while two more free and re-create pictures of their own.  No pixels (tests/ -m gpu).
// `lanczos_from_yuv_stress unregistered`: a build without a launcher unit — the entries answer CHV_ERR_NOT_IMPLEMENTED after validation.
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

static const int kChunkNV12 = 83, kChunkY420P = 62;       // include/chipvideo.h states the counts
static int chunk_of(int fmt) { return fmt == CHV_FMT_NV12 ? kChunkNV12 : kChunkY420P; }

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
    } else if (fmt == CHV_FMT_Y420P) {
        CK(chv_buffer_alloc(c, (size_t)w * h + (size_t)2 * cw * ch, &p.buf));
        p.img.n_planes = 3;
        p.img.planes[0] = chv_plane{ p.buf, 0, w, h, w, 1 };
        p.img.planes[1] = chv_plane{ p.buf, (size_t)w * h, cw, ch, cw, 1 };
        p.img.planes[2] = chv_plane{ p.buf, (size_t)w * h + (size_t)cw * ch, cw, ch, cw, 1 };
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
static unsigned long long launches() {
    unsigned long long v = 0;
    CK(chv_debug_get_counter("lanczos_from_yuv_launches", &v));
    return v;
}

struct List {
    std::vector<Pic> src, dst;
    std::vector<chv_image> ss, ds;
    int n;
};
// n pictures of 96 x 48 (+ salt) into targets of w x h
static List make_list(chv_context *c, int sfmt, int dfmt, int n, int w = 64, int h = 32, int salt = 0) {
    List l; l.n = n;
    for (int i = 0; i < n; i++) {
        l.src.push_back(make_pic(c, sfmt, 96 + 2 * salt, 48 + 2 * salt)); l.ss.push_back(l.src.back().img);
        l.dst.push_back(make_pic(c, dfmt, w, h)); l.ds.push_back(l.dst.back().img);
    }
    return l;
}
static void free_list(List &l) {
    for (Pic &p : l.src) CK(chv_buffer_free(p.buf));
    for (Pic &p : l.dst) CK(chv_buffer_free(p.buf));
}

// a list run `times` times; the stamps say every picture was reached once per run
static void run_list(chv_context *c, int sfmt, int dfmt, int n, int times, bool count, int csc) {
    List l = make_list(c, sfmt, dfmt, n);
    chv_kernel_opts opts; memset(&opts, 0, sizeof opts); opts.colorspace = csc;
    const unsigned long long before = launches();
    for (int t = 0; t < times; t++) CK(chv_scale_lanczos_from_yuv_batch(c, l.ds.data(), l.ss.data(), n, csc < 0 ? nullptr : &opts));
    if (count) EXPECT(launches() - before == (unsigned long long)times * ((n + chunk_of(sfmt) - 1) / chunk_of(sfmt)));
    CK(chv_pass_end(c, 1));
    for (const Pic &p : l.dst) EXPECT(first_byte(c, p) == (uint8_t)(0xCD + times));
    free_list(l);
}

// a fresh geometry per call (four tables each), nobody waits in between: evicted tables are retired while launches that use them are queued,
// and the list that comes back last finds its own tables evicted
static void churn(chv_context *c, int sfmt, int salt) {
    std::vector<List> ls;
    for (int k = 0; k < 40; k++) {
        ls.push_back(make_list(c, sfmt, k & 1 ? CHV_FMT_RGBA : CHV_FMT_BGRA, 2, 20 + k + 40 * (salt % 3), 10 + k, k % 7));
        CK(chv_scale_lanczos_from_yuv_batch(c, ls.back().ds.data(), ls.back().ss.data(), 2, nullptr));
    }
    CK(chv_scale_lanczos_from_yuv(c, &ls[0].ds[0], &ls[0].ss[0], nullptr));
    CK(chv_pass_end(c, 1));
    for (size_t k = 0; k < ls.size(); k++)
        for (size_t i = 0; i < ls[k].dst.size(); i++) EXPECT(first_byte(c, ls[k].dst[i]) == (uint8_t)(0xCD + (k == 0 && i == 0 ? 2 : 1)));
    for (List &l : ls) free_list(l);
}

static void singles(chv_context *c) {
    for (int sfmt : { CHV_FMT_NV12, CHV_FMT_Y420P })
        for (int dfmt : { CHV_FMT_BGRA, CHV_FMT_RGBA })
            for (int csc = -1; csc < 4; csc++) {
                Pic s = make_pic(c, sfmt, 96, 48), d = make_pic(c, dfmt, 64, 32);
                chv_kernel_opts opts; memset(&opts, 0, sizeof opts); opts.colorspace = csc;
                const unsigned long long before = launches();
                CK(chv_scale_lanczos_from_yuv(c, &d.img, &s.img, csc < 0 ? nullptr : &opts));
                EXPECT(launches() - before == 1);
                CK(chv_pass_end(c, 1));
                EXPECT(first_byte(c, d) == (uint8_t)(0xCD + 1));
                CK(chv_buffer_free(s.buf)); CK(chv_buffer_free(d.buf));
            }
    // degenerate sizes: 1 x 1 chroma planes, a 1 x 1 target
    Pic s = make_pic(c, CHV_FMT_NV12, 1, 1), d = make_pic(c, CHV_FMT_BGRA, 5, 3), s2 = make_pic(c, CHV_FMT_Y420P, 5, 3), d2 = make_pic(c, CHV_FMT_RGBA, 1, 1);
    CK(chv_scale_lanczos_from_yuv(c, &d.img, &s.img, nullptr));
    CK(chv_scale_lanczos_from_yuv(c, &d2.img, &s2.img, nullptr));
    CK(chv_pass_end(c, 1));
    EXPECT(first_byte(c, d) == (uint8_t)(0xCD + 1) && first_byte(c, d2) == (uint8_t)(0xCD + 1));
    for (Pic *p : { &s, &d, &s2, &d2 }) CK(chv_buffer_free(p->buf));
}

static void refusals(chv_context *c) {
    List x = make_list(c, CHV_FMT_NV12, CHV_FMT_BGRA, 2), y = make_list(c, CHV_FMT_Y420P, CHV_FMT_RGBA, 2);
    Pic wide = make_pic(c, CHV_FMT_NV12, 100, 48), small = make_pic(c, CHV_FMT_BGRA, 60, 32), bs = make_pic(c, CHV_FMT_BGRA, 96, 48);
    const unsigned long long before = launches();
    // the target
    EXPECT(chv_scale_lanczos_from_yuv(c, &x.ss[0], &x.ss[1], nullptr) == CHV_ERR_BAD_TARGET);                  // an NV12 target
    EXPECT(chv_scale_lanczos_from_yuv(c, &y.ss[0], &x.ss[1], nullptr) == CHV_ERR_BAD_TARGET);
    EXPECT(chv_scale_lanczos_from_yuv(c, nullptr, &x.ss[0], nullptr) == CHV_ERR_BAD_TARGET);
    chv_image bad = x.ds[0]; bad.format = CHV_FMT_NV12;
    EXPECT(chv_scale_lanczos_from_yuv(c, &bad, &x.ss[0], nullptr) == CHV_ERR_BAD_TARGET);
    bad = x.ds[0]; bad.n_planes = 2;
    EXPECT(chv_scale_lanczos_from_yuv(c, &bad, &x.ss[0], nullptr) == CHV_ERR_BAD_TARGET);
    bad = x.ds[0]; bad.planes[0].height = 1 << 20;
    EXPECT(chv_scale_lanczos_from_yuv(c, &bad, &x.ss[0], nullptr) == CHV_ERR_BAD_TARGET);
    bad = x.ds[0]; bad.planes[0].pitch = 3;
    EXPECT(chv_scale_lanczos_from_yuv(c, &bad, &x.ss[0], nullptr) == CHV_ERR_BAD_TARGET);
    bad = x.ds[0]; bad.planes[0].components = 1;
    EXPECT(chv_scale_lanczos_from_yuv(c, &bad, &x.ss[0], nullptr) == CHV_ERR_BAD_TARGET);
    // the source
    EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], &bs.img, nullptr) == CHV_ERR_BAD_INPUT);                    // a BGRA source
    EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], nullptr, nullptr) == CHV_ERR_BAD_INPUT);
    chv_image src = x.ss[0]; src.n_planes = 3;
    EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], &src, nullptr) == CHV_ERR_BAD_INPUT);
    src = y.ss[0]; src.planes[2].width -= 1;                                                                   // unequal chroma planes
    EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], &src, nullptr) == CHV_ERR_BAD_INPUT);
    src = y.ss[0]; src.planes[1].height -= 1; src.planes[2].height -= 1;                                       // equal, but not half the luma plane
    EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], &src, nullptr) == CHV_ERR_BAD_INPUT);
    src = x.ss[0]; src.planes[1].width += 1;
    EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], &src, nullptr) == CHV_ERR_BAD_INPUT);
    src = x.ss[0]; src.planes[1].components = 1;
    EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], &src, nullptr) == CHV_ERR_BAD_INPUT);
    src = x.ss[0]; src.planes[0].offset += (size_t)1 << 30;
    EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], &src, nullptr) == CHV_ERR_BAD_INPUT);
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), &src, 1, nullptr) == CHV_ERR_BAD_INPUT);
    // lists
    CK(chv_scale_lanczos_from_yuv_batch(c, nullptr, nullptr, 0, nullptr));                                     // an empty list is a no-op
    CK(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), x.ss.data(), 0, nullptr));
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), x.ss.data(), -1, nullptr) == CHV_ERR_INVALID_VALUE);
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, nullptr, x.ss.data(), 2, nullptr) == CHV_ERR_INVALID_VALUE);
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), nullptr, 2, nullptr) == CHV_ERR_INVALID_VALUE);
    chv_image d2[2] = { x.ds[0], y.ds[1] };                                                                    // two target orders
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, d2, x.ss.data(), 2, nullptr) == CHV_ERR_INVALID_VALUE);
    chv_image s2[2] = { x.ss[0], y.ss[1] };                                                                    // two source formats
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), s2, 2, nullptr) == CHV_ERR_INVALID_VALUE);
    chv_image s3[2] = { x.ss[0], wide.img };                                                                   // two source sizes
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), s3, 2, nullptr) == CHV_ERR_INVALID_VALUE);
    chv_image d3[2] = { x.ds[0], small.img };                                                                  // two target sizes
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, d3, x.ss.data(), 2, nullptr) == CHV_ERR_INVALID_VALUE);
    chv_image d4[2] = { x.ds[0], x.ds[1] }; d4[1].planes[0].height = 1 << 20;                                  // a bad plane in the LAST pair
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, d4, x.ss.data(), 2, nullptr) == CHV_ERR_BAD_TARGET);
    // 24:1, which the 160 KB rule refuses
    Pic big = make_pic(c, CHV_FMT_NV12, 96, 96), tiny = make_pic(c, CHV_FMT_BGRA, 4, 4);
    EXPECT(chv_scale_lanczos_from_yuv(c, &tiny.img, &big.img, nullptr) == CHV_ERR_INVALID_VALUE);
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, &tiny.img, &big.img, 1, nullptr) == CHV_ERR_INVALID_VALUE);
    // the other Lanczos entries keep refusing the pair
    EXPECT(chv_scale_lanczos(c, &x.ds[0], &x.ss[0]) == CHV_ERR_BAD_INPUT);
    EXPECT(launches() == before);
    // an injected launch failure: an error, nothing counted; the next call works
    stubhip_fail_launch_after(1);
    EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], &x.ss[0], nullptr) != CHV_OK);
    stubhip_fail_launch_after(1);
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), x.ss.data(), 2, nullptr) != CHV_OK);
    EXPECT(launches() == before);
    CK(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), x.ss.data(), 2, nullptr));
    EXPECT(launches() == before + 1);
    CK(chv_pass_end(c, 1));
    for (const Pic &p : x.dst) EXPECT(first_byte(c, p) == (uint8_t)(0xCD + 1));
    for (const Pic &p : y.dst) EXPECT(first_byte(c, p) == 0xCD);
    EXPECT(first_byte(c, tiny) == 0xCD && first_byte(c, small) == 0xCD);
    // the second chunk's launch fails: the first chunk was launched and counted
    List z = make_list(c, CHV_FMT_Y420P, CHV_FMT_BGRA, kChunkY420P + 1);
    stubhip_fail_launch_after(2);
    EXPECT(chv_scale_lanczos_from_yuv_batch(c, z.ds.data(), z.ss.data(), z.n, nullptr) != CHV_OK);
    EXPECT(launches() == before + 2);
    CK(chv_pass_end(c, 1));
    EXPECT(first_byte(c, z.dst[0]) == (uint8_t)(0xCD + 1) && first_byte(c, z.dst[kChunkY420P]) == 0xCD);
    free_list(x); free_list(y); free_list(z);
    for (Pic *p : { &wide, &small, &bs, &big, &tiny }) CK(chv_buffer_free(p->buf));
}

// the call inside a pass: held work is flushed in front of it, and the pass goes on
static void inside_a_pass(chv_context *c) {
    List l = make_list(c, CHV_FMT_NV12, CHV_FMT_BGRA, 2);
    CK(chv_pass_begin(c));
    CK(chv_run_kernel(c, CHV_K_IMG_CLEAR_NV12, &l.ss[0], nullptr, 0, nullptr, 0, 0, nullptr));
    CK(chv_scale_lanczos_from_yuv_batch(c, l.ds.data(), l.ss.data(), 2, nullptr));
    CK(chv_scale_lanczos_from_yuv(c, &l.ds[0], &l.ss[0], nullptr));
    CK(chv_pass_end(c, 1));
    for (size_t k = 0; k < l.dst.size(); k++) EXPECT(first_byte(c, l.dst[k]) == (uint8_t)(0xCD + (k == 0 ? 2 : 1)));
    free_list(l);
}

static void worker(int device, int id) {
    chv_context *c = nullptr;
    CK(chv_context_create(device, &c));
    const int sfmt = id & 1 ? CHV_FMT_Y420P : CHV_FMT_NV12, dfmt = id & 2 ? CHV_FMT_RGBA : CHV_FMT_BGRA;
    for (int rep = 0; rep < 3; rep++) {
        run_list(c, sfmt, dfmt, chunk_of(sfmt) + 1 + rep, 2, false, (id + rep) % 4);
        churn(c, sfmt, id + rep);
    }
    CK(chv_context_destroy(c));
}

// pictures of its own, made, converted once and freed without a wait of its own (chv_buffer_free waits for the device), while the workers run
static void recreator(int device, std::atomic<bool> *stop) {
    chv_context *c = nullptr;
    CK(chv_context_create(device, &c));
    for (int r = 0; !stop->load() || r < 20; r++) {
        List l = make_list(c, r & 1 ? CHV_FMT_NV12 : CHV_FMT_Y420P, r % 3 ? CHV_FMT_BGRA : CHV_FMT_RGBA, 1 + r % 3, 30 + r % 50, 20 + r % 9, r % 5);
        if (r & 4) CK(chv_scale_lanczos_from_yuv(c, &l.ds[0], &l.ss[0], nullptr));
        else CK(chv_scale_lanczos_from_yuv_batch(c, l.ds.data(), l.ss.data(), l.n, nullptr));
        free_list(l);
        if (r > 4000) break;
    }
    CK(chv_context_destroy(c));
}

int main(int argc, char **argv) {
    chv_context *c = nullptr;
    CK(chv_context_create(0, &c));
    if (argc > 1 && !strcmp(argv[1], "unregistered")) {
        List x = make_list(c, CHV_FMT_NV12, CHV_FMT_BGRA, 2), y = make_list(c, CHV_FMT_Y420P, CHV_FMT_RGBA, 2);
        EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], &x.ss[0], nullptr) == CHV_ERR_NOT_IMPLEMENTED);
        EXPECT(chv_scale_lanczos_from_yuv(c, &y.ds[0], &y.ss[0], nullptr) == CHV_ERR_NOT_IMPLEMENTED);
        EXPECT(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), x.ss.data(), 2, nullptr) == CHV_ERR_NOT_IMPLEMENTED);
        EXPECT(chv_scale_lanczos_from_yuv(c, &x.ss[0], &x.ss[1], nullptr) == CHV_ERR_BAD_TARGET);             // (validation comes first)
        EXPECT(chv_scale_lanczos_from_yuv(c, &x.ds[0], &x.ds[1], nullptr) == CHV_ERR_BAD_INPUT);
        chv_image s2[2] = { x.ss[0], y.ss[1] };
        EXPECT(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), s2, 2, nullptr) == CHV_ERR_INVALID_VALUE);
        CK(chv_scale_lanczos_from_yuv_batch(c, x.ds.data(), x.ss.data(), 0, nullptr));
        CK(chv_pass_end(c, 1));
        for (const Pic &p : x.dst) EXPECT(first_byte(c, p) == 0xCD);
        EXPECT(launches() == 0);
        free_list(x); free_list(y);
        CK(chv_context_destroy(c));
        printf("lanczos_from_yuv_stress: not implemented without a launcher, ok\n");
        return 0;
    }
    const int threads = argc > 1 ? atoi(argv[1]) : 6;
    for (int sfmt : { CHV_FMT_NV12, CHV_FMT_Y420P }) {
        for (int dfmt : { CHV_FMT_BGRA, CHV_FMT_RGBA }) {
            run_list(c, sfmt, dfmt, 1, 2, true, -1);
            run_list(c, sfmt, dfmt, 3, 2, true, 1);
            run_list(c, sfmt, dfmt, chunk_of(sfmt), 1, true, 2);               // exactly a chunk: one launch
            run_list(c, sfmt, dfmt, chunk_of(sfmt) + 1, 2, true, 3);           // one more than a chunk
            run_list(c, sfmt, dfmt, 2 * chunk_of(sfmt) + 1, 1, true, 0);       // three chunks
        }
        churn(c, sfmt, 0);
    }
    singles(c);
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
    printf("lanczos_from_yuv_stress: ok\n");
    return 0;
}
