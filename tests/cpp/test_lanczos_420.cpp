// tests/cpp/test_lanczos_420.cpp — the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) converting between the two 4:2:0 packings with
// Lanczos-3 (scaleLanczos420): a ladder of three rungs — two on the wave-per-strip route, one on the tile route — of two pictures into the OTHER
// packing in two launches == the same six conversions one by one; at equal sizes the conversion is an exact repack of the source's bytes;
// PictureFilter takes the pair only with convert420 set; a BGRA source and nine rungs are errors that launch nothing.  Built and run by
// tests/test_cpp_lanczos_420.py.
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
// logical chroma texel (x, y) of component c (0 Cb, 1 Cr) of a downloaded nv12 or y420p picture
static uint8_t chroma(const sv::PictureSample &s, int c, int x, int y) {
    if (s.img->planes.size() == 2) return s.img->buffers[1]->data()[(size_t)y * s.img->planes[1].stride + (size_t)2 * x + c];
    return s.img->buffers[(size_t)1 + c]->data()[(size_t)y * s.img->planes[(size_t)1 + c].stride + x];
}
static bool sameLogicalPlanes(const sv::PictureSample &a, const sv::PictureSample &b, int w, int h) {
    for (int y = 0; y < h; y++)
        if (std::memcmp(a.img->buffers[0]->data() + (size_t)y * a.img->planes[0].stride, b.img->buffers[0]->data() + (size_t)y * b.img->planes[0].stride, (size_t)w)) return false;
    for (int c = 0; c < 2; c++)
        for (int y = 0; y < h / 2; y++)
            for (int x = 0; x < w / 2; x++)
                if (chroma(a, c, x, y) != chroma(b, c, x, y)) return false;
    return true;
}
static unsigned long long launches() {
    unsigned long long v = 0;
    if (chv_debug_get_counter("lanczos_420_ladder_launches", &v)) g_fail++;
    return v;
}

int main() {
    sv::ComputeContext ctx = sv::makeComputeContext(sv::ComputeDeviceType::GPU);
    const int iw = 192, ih = 108, n = 2;
    const int sizes[3][2] = { { 128, 72 }, { 64, 36 }, { 48, 26 } };      // 10 and 18 taps; 24 / 26 taps: the tile route
    for (sv::PixelFormat f : { sv::PixelFormat::nv12, sv::PixelFormat::y420p }) {
        const sv::PixelFormat g = f == sv::PixelFormat::nv12 ? sv::PixelFormat::y420p : sv::PixelFormat::nv12;
        std::vector<sv::PictureSample> srcs;
        std::vector<std::vector<sv::PictureSample>> rungs(3), singles(3);
        for (int i = 0; i < n; i++) srcs.push_back(sv::uploadComputePicture(ctx, randomPicture(f, iw, ih, 100 + i)));
        for (int r = 0; r < 3; r++)
            for (int i = 0; i < n; i++) {
                rungs[(size_t)r].push_back(sv::uploadComputePicture(ctx, randomPicture(g, sizes[r][0], sizes[r][1], 300 + 8 * r + i)));
                singles[(size_t)r].push_back(sv::uploadComputePicture(ctx, randomPicture(g, sizes[r][0], sizes[r][1], 200 + 8 * r + i)));
            }
        unsigned long long before = launches();
        for (int r = 0; r < 3; r++)
            for (int i = 0; i < n; i++) {
                const sv::PictureSample &d = singles[(size_t)r][(size_t)i], &s = srcs[(size_t)i];
                ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczos420(c, d, s); });
            }
        EXPECT(launches() - before == 6);
        before = launches();
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczos420(c, rungs, srcs); });
        EXPECT(launches() - before == 2);
        for (int r = 0; r < 3; r++)
            for (int i = 0; i < n; i++) {
                sv::PictureSample one = sv::downloadComputePicture(ctx, singles[(size_t)r][(size_t)i], true), many = sv::downloadComputePicture(ctx, rungs[(size_t)r][(size_t)i], true);
                EXPECT(samePlanes(one, many));
                EXPECT(!samePlanes(many, randomPicture(g, sizes[r][0], sizes[r][1], 300 + 8 * r + i)));          // (the ladder wrote the target)
            }
        // at equal sizes: an exact repack, through the call and through PictureFilter with convert420
        sv::PictureSample host = randomPicture(f, iw, ih, 100);
        sv::PictureSample same = sv::uploadComputePicture(ctx, randomPicture(g, iw, ih, 500));
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczos420(c, same, srcs[0]); });
        EXPECT(sameLogicalPlanes(sv::downloadComputePicture(ctx, same, true), host, iw, ih));
        sv::PictureFilter filter({ (float)iw, (float)ih }, g, ctx, sv::PictureFilter::Scaler::lanczos);
        EXPECT(filter(srcs[0]).kind != sv::EventBox<sv::PictureSample>::just);                                    // (off by default: the error it always was)
        filter.convert420 = true;
        sv::EventBox<sv::PictureSample> out = filter(srcs[0]);
        EXPECT(out.kind == sv::EventBox<sv::PictureSample>::just);
        if (out.kind == sv::EventBox<sv::PictureSample>::just) EXPECT(sameLogicalPlanes(sv::downloadComputePicture(ctx, out.value, true), host, iw, ih));
        // an empty ladder is a no-op; a BGRA source and nine rungs are errors that launch nothing
        before = launches();
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczos420(c, std::vector<std::vector<sv::PictureSample>>{}, std::vector<sv::PictureSample>{}); });
        bool threw = false;
        sv::PictureSample bgra = sv::uploadComputePicture(ctx, randomPicture(sv::PixelFormat::BGRA, iw, ih, 600));
        try { sv::scaleLanczos420(ctx, singles[0][0], bgra); } catch (const sv::ComputeError &) { threw = true; }
        EXPECT(threw);
        std::vector<std::vector<sv::PictureSample>> nine;
        for (int r = 0; r < 9; r++) nine.push_back(rungs[(size_t)(r % 3)]);
        threw = false;
        try { sv::scaleLanczos420(ctx, nine, srcs); } catch (const sv::ComputeError &) { threw = true; }
        EXPECT(threw);
        EXPECT(launches() == before);
    }
    if (g_fail) std::printf("%d failure(s)\n", g_fail);
    else std::printf("test_lanczos_420: ok\n");
    return g_fail ? 1 : 0;
}
