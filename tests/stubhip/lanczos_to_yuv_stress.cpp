// tests/stubhip/lanczos_to_yuv_stress.cpp — the host path of chv_scale_lanczos_to_yuv / chv_scale_lanczos_to_yuv_batch under sanitizers
// (tests/test_lanczos_to_yuv_sanitizers.py): chipvideo.cpp for the CPU against the stand-in runtime, whose streams execute LAZILY, and the
// stand-in launcher (stub_lanczos_to_yuv_launcher.cpp), which reads both tables' ends and touches every plane's ends when the stream gets to
// it.  Singles and batches of 170 pictures (several descriptor slots per call), 70 geometries churning the table cache past a retire batch,
// every refusal, an injected launch failure — first on one thread, then on several with a context each while two more free and re-create
// pictures of their own.  No pixels (tests/ -m gpu).
// `lanczos_to_yuv_stress unregistered`: a build without a launcher unit — the entries answer CHV_ERR_NOT_IMPLEMENTED after validation.
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

// n pictures of one geometry: singles, then the batch (n = 170: three slots), twice; the stamps say every picture was reached
static void singles_and_batch(chv_context *c, int fmt, int order, int iw, int ih, int ow, int oh, int n, const chv_kernel_opts *opts) {
    std::vector<Pic> src, dst;
    std::vector<chv_image> ds, ss;
    for (int i = 0; i < n; i++) { src.push_back(make_pic(c, order, iw, ih)); dst.push_back(make_pic(c, fmt, ow, oh)); ds.push_back(dst.back().img); ss.push_back(src.back().img); }
    for (int i = 0; i < n; i += 7) CK(chv_scale_lanczos_to_yuv(c, &ds[(size_t)i], &ss[(size_t)i], opts));
    CK(chv_scale_lanczos_to_yuv_batch(c, ds.data(), ss.data(), n, opts));
    CK(chv_scale_lanczos_to_yuv_batch(c, ds.data(), ss.data(), n, opts));
    CK(chv_pass_end(c, 1));
    for (int i = 0; i < n; i++) EXPECT(first_byte(c, dst[(size_t)i]) == (uint8_t)(0xCD + 2 + (i % 7 == 0)));
    for (Pic &p : src) CK(chv_buffer_free(p.buf));
    for (Pic &p : dst) CK(chv_buffer_free(p.buf));
}

// 70 target sizes from one source, two tables each, nobody waits in between: evicted tables are retired while launches that use them are queued
static void churn(chv_context *c, int fmt, int salt) {
    Pic src = make_pic(c, CHV_FMT_BGRA, 96, 40);
    std::vector<Pic> dst;
    for (int i = 0; i < 70; i++) {
        dst.push_back(make_pic(c, fmt, 20 + 2 * i + 2 * (salt % 3), 10 + 2 * (i % 9)));
        CK(chv_scale_lanczos_to_yuv(c, &dst.back().img, &src.img, nullptr));
    }
    CK(chv_scale_lanczos_to_yuv(c, &dst[0].img, &src.img, nullptr));
    CK(chv_pass_end(c, 1));
    EXPECT(first_byte(c, dst[0]) == (uint8_t)(0xCD + 2));
    for (int i = 1; i < 70; i++) EXPECT(first_byte(c, dst[(size_t)i]) == (uint8_t)(0xCD + 1));
    for (Pic &p : dst) CK(chv_buffer_free(p.buf));
    CK(chv_buffer_free(src.buf));
}

static void refusals(chv_context *c) {
    Pic ns = make_pic(c, CHV_FMT_NV12, 64, 36), nd = make_pic(c, CHV_FMT_NV12, 32, 18), yd = make_pic(c, CHV_FMT_Y420P, 32, 18);
    Pic bs = make_pic(c, CHV_FMT_BGRA, 64, 36), rs = make_pic(c, CHV_FMT_RGBA, 64, 36), bd = make_pic(c, CHV_FMT_BGRA, 32, 18), nd2 = make_pic(c, CHV_FMT_NV12, 32, 20);
    const chv_kernel_opts o709 = { CHV_CSC_BT709_LIMITED, { 0, 0, 0 } };
    EXPECT(chv_scale_lanczos_to_yuv(c, &bd.img, &bs.img, &o709) == CHV_ERR_BAD_TARGET);          // a target of BGRA
    EXPECT(chv_scale_lanczos_to_yuv(c, nullptr, &bs.img, &o709) == CHV_ERR_BAD_TARGET);
    chv_image one = nd.img; one.n_planes = 1;
    EXPECT(chv_scale_lanczos_to_yuv(c, &one, &bs.img, &o709) == CHV_ERR_BAD_TARGET);
    chv_image far = nd.img; far.planes[1].height = 1 << 20;
    EXPECT(chv_scale_lanczos_to_yuv(c, &far, &bs.img, &o709) == CHV_ERR_BAD_TARGET);
    chv_image odd = yd.img; odd.planes[2].width = 15;                                             // a chroma plane that is not w / 2 wide
    EXPECT(chv_scale_lanczos_to_yuv(c, &odd, &bs.img, &o709) == CHV_ERR_BAD_TARGET);
    EXPECT(chv_scale_lanczos_to_yuv(c, &nd.img, &ns.img, &o709) == CHV_ERR_BAD_INPUT);            // nv12 -> nv12 is chv_scale_lanczos's
    EXPECT(chv_scale_lanczos_to_yuv(c, &nd.img, nullptr, &o709) == CHV_ERR_BAD_INPUT);
    chv_image lie = bs.img; lie.format = CHV_FMT_NV12;                                            // one 4-component plane that calls itself NV12
    EXPECT(chv_scale_lanczos_to_yuv(c, &nd.img, &lie, &o709) == CHV_ERR_BAD_INPUT);
    far = bs.img; far.planes[0].offset += (size_t)1 << 30;
    EXPECT(chv_scale_lanczos_to_yuv(c, &yd.img, &far, &o709) == CHV_ERR_BAD_INPUT);
    EXPECT(chv_scale_lanczos(c, &nd.img, &bs.img) == CHV_ERR_BAD_INPUT);                          // (the plain entry keeps its answer)
    // 4000 x 2 -> 2 x 2 is beyond the table's 256 taps
    Pic wide = make_pic(c, CHV_FMT_BGRA, 4000, 2), tiny = make_pic(c, CHV_FMT_NV12, 2, 2);
    EXPECT(chv_scale_lanczos_to_yuv(c, &tiny.img, &wide.img, nullptr) == CHV_ERR_INVALID_VALUE);
    // one geometry, one source format and one target format per batch; an empty batch is a no-op
    chv_image d2[2] = { nd.img, yd.img }, s2[2] = { bs.img, bs.img };
    EXPECT(chv_scale_lanczos_to_yuv_batch(c, d2, s2, 2, nullptr) == CHV_ERR_INVALID_VALUE);
    chv_image d3[2] = { nd.img, nd2.img };
    EXPECT(chv_scale_lanczos_to_yuv_batch(c, d3, s2, 2, nullptr) == CHV_ERR_INVALID_VALUE);
    chv_image d4[2] = { nd.img, nd.img }, s4[2] = { bs.img, rs.img };
    EXPECT(chv_scale_lanczos_to_yuv_batch(c, d4, s4, 2, nullptr) == CHV_ERR_INVALID_VALUE);
    EXPECT(chv_scale_lanczos_to_yuv_batch(c, &bd.img, &bs.img, 1, nullptr) == CHV_ERR_BAD_TARGET);
    EXPECT(chv_scale_lanczos_to_yuv_batch(c, &nd.img, &ns.img, 1, nullptr) == CHV_ERR_BAD_INPUT);
    EXPECT(chv_scale_lanczos_to_yuv_batch(c, &nd.img, &bs.img, -1, nullptr) == CHV_ERR_INVALID_VALUE);
    CK(chv_scale_lanczos_to_yuv_batch(c, nullptr, nullptr, 0, nullptr));
    // an injected launch failure comes back as an error; the next call works
    stubhip_fail_launch_after(1);
    EXPECT(chv_scale_lanczos_to_yuv(c, &nd.img, &bs.img, &o709) != CHV_OK);
    CK(chv_scale_lanczos_to_yuv(c, &nd.img, &bs.img, &o709));
    CK(chv_scale_lanczos_to_yuv(c, &yd.img, &rs.img, nullptr));
    CK(chv_pass_end(c, 1));
    EXPECT(first_byte(c, nd) == (uint8_t)(0xCD + 1) && first_byte(c, yd) == (uint8_t)(0xCD + 1) && first_byte(c, tiny) == 0xCD && first_byte(c, nd2) == 0xCD);
    EXPECT(first_byte(c, bd) == 0xCD);
    for (Pic *p : { &ns, &nd, &yd, &bs, &rs, &bd, &nd2, &wide, &tiny }) CK(chv_buffer_free(p->buf));
}

// the conversion inside a pass: held work is flushed in front of it, and the pass goes on
static void inside_a_pass(chv_context *c) {
    Pic bs = make_pic(c, CHV_FMT_BGRA, 64, 36), nd = make_pic(c, CHV_FMT_NV12, 32, 18);
    CK(chv_pass_begin(c));
    CK(chv_run_kernel(c, CHV_K_IMG_CLEAR_BGRA, &bs.img, nullptr, 0, nullptr, 0, 0, nullptr));
    CK(chv_scale_lanczos_to_yuv(c, &nd.img, &bs.img, nullptr));
    CK(chv_pass_end(c, 1));
    EXPECT(first_byte(c, nd) == (uint8_t)(0xCD + 1));
    CK(chv_buffer_free(bs.buf)); CK(chv_buffer_free(nd.buf));
}

static void worker(int device, int id) {
    chv_context *c = nullptr;
    CK(chv_context_create(device, &c));
    const int fmt = id & 1 ? CHV_FMT_Y420P : CHV_FMT_NV12;
    const chv_kernel_opts o = { id & 3, { 0, 0, 0 } };
    for (int rep = 0; rep < 3; rep++) {
        singles_and_batch(c, fmt, id & 2 ? CHV_FMT_RGBA : CHV_FMT_BGRA, 40, 24, 20, 12, 170, &o);
        churn(c, fmt, id + rep);
    }
    CK(chv_context_destroy(c));
}

// pictures of its own, made, converted once and freed without a wait of its own (chv_buffer_free waits for the device), while the workers run
static void recreator(int device, std::atomic<bool> *stop) {
    chv_context *c = nullptr;
    CK(chv_context_create(device, &c));
    for (int r = 0; !stop->load() || r < 20; r++) {
        Pic s = make_pic(c, CHV_FMT_BGRA, 50 + r % 5, 22), d = make_pic(c, r & 1 ? CHV_FMT_NV12 : CHV_FMT_Y420P, 24, 14);
        CK(chv_scale_lanczos_to_yuv(c, &d.img, &s.img, nullptr));
        CK(chv_buffer_free(s.buf));
        CK(chv_buffer_free(d.buf));
        if (r > 4000) break;
    }
    CK(chv_context_destroy(c));
}

int main(int argc, char **argv) {
    chv_context *c = nullptr;
    CK(chv_context_create(0, &c));
    if (argc > 1 && !strcmp(argv[1], "unregistered")) {
        Pic bs = make_pic(c, CHV_FMT_BGRA, 64, 36), nd = make_pic(c, CHV_FMT_NV12, 32, 18), yd = make_pic(c, CHV_FMT_Y420P, 32, 18), bd = make_pic(c, CHV_FMT_BGRA, 32, 18);
        EXPECT(chv_scale_lanczos_to_yuv(c, &nd.img, &bs.img, nullptr) == CHV_ERR_NOT_IMPLEMENTED);
        EXPECT(chv_scale_lanczos_to_yuv(c, &yd.img, &bs.img, nullptr) == CHV_ERR_NOT_IMPLEMENTED);
        EXPECT(chv_scale_lanczos_to_yuv_batch(c, &nd.img, &bs.img, 1, nullptr) == CHV_ERR_NOT_IMPLEMENTED);
        EXPECT(chv_scale_lanczos_to_yuv_batch(c, &yd.img, &bs.img, 1, nullptr) == CHV_ERR_NOT_IMPLEMENTED);
        EXPECT(chv_scale_lanczos_to_yuv(c, &bd.img, &bs.img, nullptr) == CHV_ERR_BAD_TARGET);          // (validation comes first)
        EXPECT(chv_scale_lanczos_to_yuv(c, &nd.img, &nd.img, nullptr) == CHV_ERR_BAD_INPUT);
        CK(chv_scale_lanczos(c, &bd.img, &bs.img));
        CK(chv_pass_end(c, 1));
        EXPECT(first_byte(c, nd) == 0xCD && first_byte(c, yd) == 0xCD);
        for (Pic *p : { &bs, &nd, &yd, &bd }) CK(chv_buffer_free(p->buf));
        CK(chv_context_destroy(c));
        printf("lanczos_to_yuv_stress: not implemented without a launcher, ok\n");
        return 0;
    }
    const int threads = argc > 1 ? atoi(argv[1]) : 6;
    const chv_kernel_opts full = { CHV_CSC_BT709_FULL, { 0, 0, 0 } };
    for (int fmt : { CHV_FMT_NV12, CHV_FMT_Y420P }) {
        singles_and_batch(c, fmt, CHV_FMT_BGRA, 40, 24, 20, 12, 170, nullptr);          // 83 + 83 + 4 / 62 + 62 + 46 pictures per slot
        singles_and_batch(c, fmt, CHV_FMT_RGBA, 40, 24, 20, 12, fmt == CHV_FMT_NV12 ? 84 : 63, &full);      // one more than a chunk
        singles_and_batch(c, fmt, CHV_FMT_BGRA, 146, 20, 73, 10, 5, &full);
        singles_and_batch(c, fmt, CHV_FMT_RGBA, 2, 2, 7, 5, 3, nullptr);
        singles_and_batch(c, fmt, CHV_FMT_BGRA, 5, 3, 1, 1, 2, nullptr);
        churn(c, fmt, 0);
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
    printf("lanczos_to_yuv_stress: ok\n");
    return 0;
}
