// tests/cpp/test_lanczos_planar_ladder.cpp — the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) making a 4:2:0 encoder ladder with
// Lanczos-3 (scaleLanczos(ctx, rungs, srcs)): four rungs — three on the wave-per-strip route, one on the tile route — of two nv12 or y420p
// pictures == the same eight resizes one by one; an empty ladder is a no-op; a rung with a missing target, nine rungs and sources of the other
// format are errors that launch nothing.  Built and run by tests/test_cpp_lanczos_planar_ladder.py.
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
static unsigned long long launches() {
    unsigned long long v = 0;
    if (chv_debug_get_counter("lanczos_planar_ladder_launches", &v)) g_fail++;
    return v;
}

int main() {
    sv::ComputeContext ctx = sv::makeComputeContext(sv::ComputeDeviceType::GPU);
    const int iw = 192, ih = 108, n = 2;
    const int sizes[4][2] = { { 128, 72 }, { 96, 54 }, { 64, 36 }, { 48, 26 } };      // 10, 12 and 18 taps; 24 / 26 taps: the tile route
    for (sv::PixelFormat f : { sv::PixelFormat::nv12, sv::PixelFormat::y420p }) {
        std::vector<sv::PictureSample> srcs;
        std::vector<std::vector<sv::PictureSample>> rungs(4), singles(4);
        for (int i = 0; i < n; i++) srcs.push_back(sv::uploadComputePicture(ctx, randomPicture(f, iw, ih, 100 + i)));
        for (int r = 0; r < 4; r++)
            for (int i = 0; i < n; i++) {
                rungs[(size_t)r].push_back(sv::uploadComputePicture(ctx, randomPicture(f, sizes[r][0], sizes[r][1], 300 + 8 * r + i)));
                singles[(size_t)r].push_back(sv::uploadComputePicture(ctx, randomPicture(f, sizes[r][0], sizes[r][1], 200 + 8 * r + i)));
            }
        for (int r = 0; r < 4; r++)
            for (int i = 0; i < n; i++) {
                const sv::PictureSample &d = singles[(size_t)r][(size_t)i], &s = srcs[(size_t)i];
                ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczos(c, d, s); });
            }
        const unsigned long long before = launches();
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczos(c, rungs, srcs); });
        EXPECT(launches() - before == 2);
        for (int r = 0; r < 4; r++)
            for (int i = 0; i < n; i++) {
                sv::PictureSample one = sv::downloadComputePicture(ctx, singles[(size_t)r][(size_t)i], true), many = sv::downloadComputePicture(ctx, rungs[(size_t)r][(size_t)i], true);
                EXPECT(samePlanes(one, many));
                EXPECT(!samePlanes(many, randomPicture(f, sizes[r][0], sizes[r][1], 300 + 8 * r + i)));          // (the ladder wrote the target)
            }
        // an empty ladder is a no-op
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczos(c, std::vector<std::vector<sv::PictureSample>>{}, std::vector<sv::PictureSample>{}); });
        // a rung with a missing target, and nine rungs: errors, nothing launched
        std::vector<std::vector<sv::PictureSample>> shortRung = rungs;
        shortRung[3].pop_back();
        bool threw = false;
        try { sv::scaleLanczos(ctx, shortRung, srcs); } catch (const sv::ComputeError &) { threw = true; }
        EXPECT(threw);
        std::vector<std::vector<sv::PictureSample>> nine;
        for (int r = 0; r < 9; r++) nine.push_back(rungs[(size_t)(r % 4)]);
        threw = false;
        try { sv::scaleLanczos(ctx, nine, srcs); } catch (const sv::ComputeError &) { threw = true; }
        EXPECT(threw);
        std::vector<sv::PictureSample> others;          // sources of the other 4:2:0 format
        for (int i = 0; i < n; i++) others.push_back(sv::uploadComputePicture(ctx, randomPicture(f == sv::PixelFormat::nv12 ? sv::PixelFormat::y420p : sv::PixelFormat::nv12, iw, ih, 400 + i)));
        threw = false;
        try { sv::scaleLanczos(ctx, rungs, others); } catch (const sv::ComputeError &) { threw = true; }
        EXPECT(threw);
        EXPECT(launches() - before == 2);
    }
    if (g_fail) std::printf("%d failure(s)\n", g_fail);
    else std::printf("test_lanczos_planar_ladder: ok\n");
    return g_fail ? 1 : 0;
}
