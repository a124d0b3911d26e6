// tests/cpp/test_lanczos_rgb_ladder.cpp — the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) making every rendition of a list of
// BGRA and RGBA pictures with one call (scaleLanczosRgbLadder): a ladder of four rungs — three on the wave-per-strip route, one on the tile
// route — over two pictures leaves in two launches and holds the bytes of the eight single calls; two rungs of one size hold the same
// bytes; an empty ladder is a no-op; a rung with a missing target, an nv12 source and an nv12 target are errors that launch nothing.
// Built and run by tests/test_cpp_lanczos_rgb_ladder.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../swiftvideo_amd/host/swiftvideo_hip.hpp"

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } } while (0)

// splitmix64 low bytes, as tests/util.py
static void fill(sv::Data &d, uint64_t seed) {
    uint64_t x = seed;
    for (auto &b : d) {
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        b = (uint8_t)z;
    }
}
static sv::PictureSample randomPicture(sv::PixelFormat f, int w, int h, uint64_t seed) {
    sv::PictureSample s = sv::createPictureSample({ (float)w, (float)h }, f, "cam");
    for (size_t i = 0; i < s.img->buffers.size(); i++) fill(*s.img->buffers[i], seed * 16 + i);
    return s;
}
static bool samePlanes(const sv::PictureSample &a, const sv::PictureSample &b) {
    if (a.img->planes.size() != b.img->planes.size()) return false;
    for (size_t i = 0; i < a.img->planes.size(); i++) {
        const sv::Plane &p = a.img->planes[i];
        size_t row = (size_t)p.size.x * sv::planeComponents(p);
        for (int y = 0; y < (int)p.size.y; y++)
            if (std::memcmp(a.img->buffers[i]->data() + (size_t)y * p.stride, b.img->buffers[i]->data() + (size_t)y * p.stride, row)) return false;
    }
    return true;
}
static unsigned long long counter(const char *name) {
    unsigned long long v = 0;
    if (chv_debug_get_counter(name, &v)) g_fail++;
    return v;
}
static unsigned long long launches() { return counter("lanczos_rgb_ladder_launches"); }

int main() {
    sv::ComputeContext ctx = sv::makeComputeContext(sv::ComputeDeviceType::GPU);
    const int iw = 192, ih = 108, n = 2;
    // 10 taps, the same size again, an enlargement: the strip route; 6:1, 36 taps: the tile route
    const int sizes[4][2] = { { 128, 72 }, { 128, 72 }, { 240, 136 }, { 32, 18 } };
    for (sv::PixelFormat order : { sv::PixelFormat::BGRA, sv::PixelFormat::RGBA }) {
        std::vector<sv::PictureSample> srcs;
        for (int i = 0; i < n; i++) srcs.push_back(sv::uploadComputePicture(ctx, randomPicture(order, iw, ih, 100 + i)));
        std::vector<std::vector<sv::PictureSample>> rungs(4), singles(4);
        for (int r = 0; r < 4; r++)
            for (int i = 0; i < n; i++) {
                rungs[(size_t)r].push_back(sv::uploadComputePicture(ctx, randomPicture(order, sizes[r][0], sizes[r][1], 300 + 8 * r + i)));
                singles[(size_t)r].push_back(sv::uploadComputePicture(ctx, randomPicture(order, sizes[r][0], sizes[r][1], 200 + 8 * r + i)));
            }
        unsigned long long before = launches(), other_before = counter("lanczos_from_yuv_ladder_launches");
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosRgbLadder(c, rungs, srcs); });
        EXPECT(launches() - before == 2);
        EXPECT(counter("lanczos_from_yuv_ladder_launches") == other_before);
        for (int r = 0; r < 4; r++)
            for (int i = 0; i < n; i++) {
                const sv::PictureSample &d = singles[(size_t)r][(size_t)i], &s = srcs[(size_t)i];
                ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczos(c, d, s); });
                sv::PictureSample one = sv::downloadComputePicture(ctx, d, true), many = sv::downloadComputePicture(ctx, rungs[(size_t)r][(size_t)i], true);
                EXPECT(samePlanes(one, many));
                EXPECT(!samePlanes(many, randomPicture(order, sizes[r][0], sizes[r][1], 300 + 8 * r + i)));       // (the ladder wrote the target)
            }
        for (int i = 0; i < n; i++)
            EXPECT(samePlanes(sv::downloadComputePicture(ctx, rungs[0][(size_t)i], true), sv::downloadComputePicture(ctx, rungs[1][(size_t)i], true)));
        EXPECT(launches() - before == 2);
        // an empty ladder is a no-op; a rung without its targets, an nv12 source and an nv12 target are errors that launch nothing
        before = launches();
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosRgbLadder(c, std::vector<std::vector<sv::PictureSample>>{}, std::vector<sv::PictureSample>{}); });
        bool threw = false;
        try { sv::scaleLanczosRgbLadder(ctx, std::vector<std::vector<sv::PictureSample>>{ rungs[0], { rungs[2][0] } }, srcs); } catch (const sv::ComputeError &) { threw = true; }
        EXPECT(threw);
        sv::PictureSample yuv = sv::uploadComputePicture(ctx, randomPicture(sv::PixelFormat::nv12, iw, ih, 400));
        threw = false;
        try { sv::scaleLanczosRgbLadder(ctx, std::vector<std::vector<sv::PictureSample>>{ rungs[0] }, std::vector<sv::PictureSample>{ srcs[0], yuv }); } catch (const sv::ComputeError &) { threw = true; }
        EXPECT(threw);
        threw = false;
        try { sv::scaleLanczosRgbLadder(ctx, std::vector<std::vector<sv::PictureSample>>{ rungs[0], { rungs[2][0], yuv } }, srcs); } catch (const sv::ComputeError &) { threw = true; }
        EXPECT(threw);
        EXPECT(launches() == before);
        for (int r = 0; r < 4; r++)       // (nothing was written by the refusals)
            for (int i = 0; i < n; i++)
                EXPECT(samePlanes(sv::downloadComputePicture(ctx, singles[(size_t)r][(size_t)i], true), sv::downloadComputePicture(ctx, rungs[(size_t)r][(size_t)i], true)));
    }
    if (g_fail) std::printf("%d failure(s)\n", g_fail);
    else std::printf("test_lanczos_rgb_ladder: ok\n");
    return g_fail ? 1 : 0;
}
