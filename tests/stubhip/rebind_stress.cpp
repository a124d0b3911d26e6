// tests/stubhip/rebind_stress.cpp — chv_batch_rebind's host logic under sanitizers (tests/test_batch_rebind_sanitizers.py): chipvideo.cpp for the
// CPU against the stand-in runtime, whose streams execute LAZILY, and the stand-in scatter launcher (stub_rebind_launcher.cpp).  The stub tick
// kernels touch the first and last byte of every plane their descriptors name and stamp the canvas (+1 on its first byte per launch), so a stale
// descriptor, a stale dependency or a list read too late is a sanitizer report or a wrong stamp.  No pixels (tests/ -m gpu).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "chipvideo.h"

void stubhip_fail_launch_after(int n);      // stub_runtime.cpp

#define CK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s:%d %s -> %s (%s)\n", __FILE__, __LINE__, #x, chv_error_string(rc_), chv_last_error_detail()); exit(2); } } while (0)
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d expectation failed: %s\n", __FILE__, __LINE__, #cond); exit(3); } } while (0)

static const int W = 256, H = 64;
struct Pic { chv_buffer *buf = nullptr; chv_image img; };
static Pic make_pic(chv_context *c, int fmt) {
    Pic p; memset(&p.img, 0, sizeof p.img);
    p.img.format = fmt; p.img.width = W; p.img.height = H;
    if (fmt == CHV_FMT_NV12) {
        CK(chv_buffer_alloc(c, (size_t)W * H * 3 / 2, &p.buf));
        p.img.n_planes = 2;
        p.img.planes[0] = chv_plane{ p.buf, 0, W, H, W, 1 };
        p.img.planes[1] = chv_plane{ p.buf, (size_t)W * H, W / 2, H / 2, W, 2 };
    } else {
        size_t pitch = 0;
        CK(chv_plane_alloc(c, W, H, 4, &p.buf, &pitch));
        p.img.n_planes = 1;
        p.img.planes[0] = chv_plane{ p.buf, 0, W, H, (int32_t)pitch, 4 };
    }
    return p;
}
static chv_uniforms full_canvas(float opacity) {
    chv_uniforms u; memset(&u, 0, sizeof u);
    const float t[16] = { .5f, 0, 0, .5f, 0, .5f, 0, .5f, 0, 0, 1, -1, 0, 0, 0, 1 }, id[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    memcpy(u.transform, t, sizeof t); memcpy(u.border_matrix, t, sizeof t); memcpy(u.texture_transform, id, sizeof id);
    u.opacity = opacity; u.output_size[0] = (float)W; u.output_size[1] = (float)H; u.input_size[0] = (float)W; u.input_size[1] = (float)H;
    return u;
}

// One picture set of a scene of `n` ticks: per tick a canvas, `videos` NV12 pictures and one BGRA overlay.  videos 4: a split batch (two
// launches per run), videos 1: one launch through the ring route with geometry tables.
struct Set {
    int n, videos;
    std::vector<Pic> canvas, vid, rgb;
    std::vector<int> stamps;        // launches that wrote each canvas
    Set(chv_context *c, int n_, int videos_) : n(n_), videos(videos_), stamps((size_t)n_, 0) {
        for (int t = 0; t < n; t++) {
            canvas.push_back(make_pic(c, CHV_FMT_BGRA)); rgb.push_back(make_pic(c, CHV_FMT_BGRA));
            for (int v = 0; v < videos; v++) vid.push_back(make_pic(c, CHV_FMT_NV12));
        }
    }
    void layers(int t, std::vector<chv_layer> &out) const {
        for (int v = 0; v <= videos; v++) {
            chv_layer l; memset(&l, 0, sizeof l);
            l.kernel = v < videos ? CHV_K_IMG_NV12_BGRA : CHV_K_IMG_BGRA_BGRA_TX;
            l.image = v < videos ? vid[(size_t)(t * videos + v)].img : rgb[(size_t)t].img;
            l.uniforms = full_canvas(1.f - .2f * v);
            out.push_back(l);
        }
    }
    chv_batch *create(chv_context *c) const {
        std::vector<std::vector<chv_layer>> ls((size_t)n);
        std::vector<chv_tick> ticks((size_t)n);
        for (int t = 0; t < n; t++) {
            layers(t, ls[(size_t)t]);
            memset(&ticks[(size_t)t], 0, sizeof(chv_tick));
            ticks[(size_t)t].target = canvas[(size_t)t].img; ticks[(size_t)t].clear_first = 1;
            ticks[(size_t)t].n_layers = videos + 1; ticks[(size_t)t].layers = ls[(size_t)t].data();
        }
        chv_batch *b = nullptr;
        CK(chv_batch_create(c, ticks.data(), n, &b));
        return b;
    }
    std::vector<chv_rebind> items() const {
        std::vector<chv_rebind> out;
        for (int t = 0; t < n; t++) {
            out.push_back(chv_rebind{ t, -1, canvas[(size_t)t].img });
            for (int v = 0; v < videos; v++) out.push_back(chv_rebind{ t, v, vid[(size_t)(t * videos + v)].img });
            out.push_back(chv_rebind{ t, videos, rgb[(size_t)t].img });
        }
        return out;
    }
    void ran(int launches) { for (int &s : stamps) s += launches; }
    void check(chv_context *c) const {
        for (int t = 0; t < n; t++) {
            uint8_t first = 0;
            CK(chv_download(c, &first, 1, canvas[(size_t)t].buf, 0, (size_t)canvas[(size_t)t].img.planes[0].pitch, 1, 1));
            EXPECT(first == (uint8_t)(0xCD + stamps[(size_t)t]));
        }
    }
    void free_all() {
        for (auto *v : { &canvas, &vid, &rgb }) { for (Pic &p : *v) CK(chv_buffer_free(p.buf)); v->clear(); }
    }
};

static int launches_of(chv_batch *b) { int nl = 0; CK(chv_batch_describe(b, nullptr, 0, &nl)); return nl; }

// rotating rings: `rounds` rebinds over `ring` picture sets, a host wait now and then, both mechanisms in turn; then buffers rebound away are
// freed once their runs have drained, and the batch runs on
static void rotate(chv_context *c, int n_ticks, int videos, int rounds, int ring) {
    std::vector<Set> sets;
    for (int k = 0; k < ring; k++) sets.emplace_back(c, n_ticks, videos);
    chv_batch *b = sets[0].create(c);
    const int nl = launches_of(b);
    EXPECT(nl == (videos >= 2 ? 2 : 1));
    CK(chv_batch_run(c, b)); sets[0].ran(nl);
    for (int r = 1; r <= rounds; r++) {
        if (r % 50 == 1) CK(chv_debug_set_switch("CHV_REBIND", (r / 50) % 2 ? "copy" : "scatter"));
        Set &s = sets[(size_t)(r % ring)];
        const std::vector<chv_rebind> it = s.items();
        CK(chv_batch_rebind(c, b, it.data(), (int)it.size()));
        CK(chv_batch_run(c, b)); s.ran(nl);
        if (r % 7 == 0) CK(chv_pass_end(c, 1));
        if (r % 11 == 0) { CK(chv_batch_run(c, b)); s.ran(nl); }
    }
    CK(chv_pass_end(c, 1));
    for (const Set &s : sets) s.check(c);
    // the batch is on set rounds % ring; every other set goes, and the batch keeps running (its dependencies are the buffers bound NOW)
    const size_t cur = (size_t)(rounds % ring);
    for (size_t k = 0; k < sets.size(); k++) if (k != cur) sets[k].free_all();
    for (int i = 0; i < 3; i++) { CK(chv_batch_run(c, b)); sets[cur].ran(nl); }
    CK(chv_pass_end(c, 1));
    sets[cur].check(c);
    // one more set, rebound to WITHOUT a wait; the old one is freed after the wait
    Set last(c, n_ticks, videos);
    const std::vector<chv_rebind> it = last.items();
    CK(chv_batch_rebind(c, b, it.data(), (int)it.size()));
    CK(chv_pass_end(c, 1));
    sets[cur].free_all();
    CK(chv_batch_run(c, b)); last.ran(nl);
    CK(chv_pass_end(c, 1));
    last.check(c);
    CK(chv_batch_destroy(b));
    last.free_all();
    CK(chv_debug_set_switch("CHV_REBIND", nullptr));
}

// an injected launch failure in the scatter: the error comes back, the batch stays on the pictures it had (the new ones are freed at once)
static void failing_scatter(chv_context *c, int n_ticks) {
    CK(chv_debug_set_switch("CHV_REBIND", "scatter"));
    Set a(c, n_ticks, 1);
    chv_batch *b = a.create(c);
    const int nl = launches_of(b);
    CK(chv_batch_run(c, b)); a.ran(nl);
    for (int rep = 0; rep < 4; rep++) {
        Set gone(c, n_ticks, 1);
        const std::vector<chv_rebind> it = gone.items();
        stubhip_fail_launch_after(1);
        EXPECT(chv_batch_rebind(c, b, it.data(), (int)it.size()) != CHV_OK);
        gone.free_all();
        CK(chv_batch_run(c, b)); a.ran(nl);
        if (rep & 1) CK(chv_pass_end(c, 1));
    }
    // ... and takes the next list
    Set next(c, n_ticks, 1);
    const std::vector<chv_rebind> it = next.items();
    CK(chv_batch_rebind(c, b, it.data(), (int)it.size()));
    CK(chv_batch_run(c, b)); next.ran(nl);
    CK(chv_pass_end(c, 1));
    a.check(c); next.check(c);
    // refusals change nothing either: a duplicate, an index out of range, a picture of another pitch behind a valid item
    std::vector<chv_rebind> bad = a.items();
    bad.push_back(bad[1]);
    EXPECT(chv_batch_rebind(c, b, bad.data(), (int)bad.size()) == CHV_ERR_INVALID_VALUE);
    bad.pop_back(); bad[2].tick = n_ticks;
    EXPECT(chv_batch_rebind(c, b, bad.data(), (int)bad.size()) == CHV_ERR_INVALID_VALUE);
    bad = a.items(); bad[(size_t)bad.size() - 1].image.planes[0].pitch += 16;
    EXPECT(chv_batch_rebind(c, b, bad.data(), (int)bad.size()) != CHV_OK);
    a.free_all();
    CK(chv_batch_run(c, b)); next.ran(nl);
    CK(chv_pass_end(c, 1));
    next.check(c);
    CK(chv_batch_destroy(b));
    next.free_all();
    CK(chv_debug_set_switch("CHV_REBIND", nullptr));
}

// destroy with a rebind in flight, then a new batch of the same size: it takes the pooled block the first one gave back
static void destroy_in_flight(chv_context *c, int n_ticks) {
    for (int rep = 0; rep < 12; rep++) {
        CK(chv_debug_set_switch("CHV_REBIND", rep % 2 ? "copy" : "scatter"));
        Set a(c, n_ticks, 4), b2(c, n_ticks, 4), n(c, n_ticks, 4);
        chv_batch *b = a.create(c);
        const int nl = launches_of(b);
        CK(chv_batch_run(c, b)); a.ran(nl);
        const std::vector<chv_rebind> it = b2.items();
        CK(chv_batch_rebind(c, b, it.data(), (int)it.size()));
        if (rep % 3) { CK(chv_batch_run(c, b)); b2.ran(nl); }
        CK(chv_batch_destroy(b));
        chv_batch *nb = n.create(c);
        CK(chv_batch_run(c, nb)); n.ran(nl);
        CK(chv_pass_end(c, 1));
        a.check(c); b2.check(c); n.check(c);
        CK(chv_batch_destroy(nb));
        a.free_all(); b2.free_all(); n.free_all();
    }
    CK(chv_debug_set_switch("CHV_REBIND", nullptr));
}

// created on one context, rebound on a second, run on a third, nobody waits in between
static void three_contexts(chv_context *c) {
    chv_context *c2 = nullptr, *c3 = nullptr;
    CK(chv_context_share(c, &c2)); CK(chv_context_share(c, &c3));
    Set a(c, 5, 4), b2(c, 5, 4);
    chv_batch *b = a.create(c);
    const int nl = launches_of(b);
    for (int r = 0; r < 40; r++) {
        Set &now = r % 2 ? a : b2;
        CK(chv_batch_run(c, b)); (r % 2 ? b2 : a).ran(nl);
        const std::vector<chv_rebind> it = now.items();
        CK(chv_batch_rebind(c2, b, it.data(), (int)it.size()));
        CK(chv_batch_run(c3, b)); now.ran(nl);
        if (r % 5 == 4) { CK(chv_pass_end(c3, 1)); }
    }
    CK(chv_pass_end(c3, 1)); CK(chv_pass_end(c, 1));
    a.check(c); b2.check(c);
    CK(chv_batch_destroy(b));
    a.free_all(); b2.free_all();
    CK(chv_context_destroy(c2)); CK(chv_context_destroy(c3));
}

static void worker(int device, int id) {
    chv_context *c = nullptr;
    CK(chv_context_create(device, &c));
    Set a(c, 4, 1 + 3 * (id & 1)), b2(c, 4, 1 + 3 * (id & 1));
    chv_batch *b = a.create(c);
    const int nl = launches_of(b);
    for (int r = 0; r < 300; r++) {
        Set &now = r % 2 ? a : b2;
        const std::vector<chv_rebind> it = now.items();
        CK(chv_batch_rebind(c, b, it.data(), (int)it.size()));
        CK(chv_batch_run(c, b)); now.ran(nl);
        if (r % 9 == 0) CK(chv_pass_end(c, 1));
    }
    CK(chv_pass_end(c, 1));
    a.check(c); b2.check(c);
    CK(chv_batch_destroy(b));
    a.free_all(); b2.free_all();
    CK(chv_context_destroy(c));
}

int main(int argc, char **argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 8;
    chv_context *c = nullptr;
    CK(chv_context_create(0, &c));
    EXPECT(strstr(chv_build_flags(), "batch_rebind:scatter=1") != nullptr);
    rotate(c, 6, 4, 2400, 4);        // 60 pairs per rebind: kernel arguments; a split batch
    rotate(c, 6, 1, 900, 3);         // one launch through the ring route: geometry tables patched into the layers between rebinds
    rotate(c, 40, 4, 240, 3);        // 560 pairs (the split doubles the targets'): the pinned lists, two in turn
    failing_scatter(c, 6);
    failing_scatter(c, 90);          // a long list: the failure comes after the pinned area was written
    destroy_in_flight(c, 6);
    destroy_in_flight(c, 40);
    three_contexts(c);
    std::vector<std::thread> pool;
    for (int i = 0; i < threads; i++) pool.emplace_back(worker, i % 2, i);
    for (auto &t : pool) t.join();
    CK(chv_context_destroy(c));
    printf("rebind_stress: ok\n");
    return 0;
}
