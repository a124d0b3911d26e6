// tests/cpp/test_lanczos_to_yuv.cpp — the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) converting BGRA pictures to nv12 and y420p with
// Lanczos-3 (scaleLanczosToYuv): a batch of three of one geometry == the same three one by one, and the PictureFilter rule: BGRA -> nv12 and
// BGRA -> y420p run and give the bytes of scaleLanczosToYuv, the float matrix has no Lanczos form, nv12 -> BGRA stays an error.  Built and run
// by tests/test_cpp_lanczos_to_yuv.py.
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

int main() {
    sv::ComputeContext ctx = sv::makeComputeContext(sv::ComputeDeviceType::GPU);
    const int iw = 96, ih = 54, ow = 64, oh = 36, csc = CHV_CSC_BT709_LIMITED;
    for (sv::PixelFormat f : { sv::PixelFormat::nv12, sv::PixelFormat::y420p }) {
        std::vector<sv::PictureSample> srcs, singles;
        std::vector<std::pair<sv::PictureSample, sv::PictureSample>> pairs;
        for (int i = 0; i < 3; i++) {
            srcs.push_back(sv::uploadComputePicture(ctx, randomPicture(sv::PixelFormat::BGRA, iw, ih, 100 + i)));
            singles.push_back(sv::uploadComputePicture(ctx, randomPicture(f, ow, oh, 200 + i)));
            pairs.emplace_back(sv::uploadComputePicture(ctx, randomPicture(f, ow, oh, 300 + i)), srcs.back());
        }
        for (int i = 0; i < 3; i++) {
            const sv::PictureSample &d = singles[(size_t)i], &s = srcs[(size_t)i];
            ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosToYuv(c, d, s, csc); });
        }
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosToYuv(c, pairs, csc); });
        for (int i = 0; i < 3; i++) {
            sv::PictureSample one = sv::downloadComputePicture(ctx, singles[(size_t)i], true), many = sv::downloadComputePicture(ctx, pairs[(size_t)i].first, true);
            EXPECT(samePlanes(one, many));
            EXPECT(!samePlanes(one, randomPicture(f, ow, oh, 200 + i)));          // (the conversion wrote the target)
        }
        // an empty list is a no-op
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosToYuv(c, std::vector<std::pair<sv::PictureSample, sv::PictureSample>>{}, csc); });
        // the filter: BGRA -> 4:2:0 runs the conversion with the filter's colourspace ...
        sv::PictureFilter filter({ (float)ow, (float)oh }, f, ctx, sv::PictureFilter::Scaler::lanczos, csc);
        auto out = filter(randomPicture(sv::PixelFormat::BGRA, iw, ih, 100));
        EXPECT(out.kind == out.just);
        if (out.kind == out.just) EXPECT(samePlanes(sv::downloadComputePicture(ctx, out.value, true), sv::downloadComputePicture(ctx, singles[0], true)));
        // ... the float full-range matrix has no Lanczos form ...
        sv::PictureFilter floatMatrix({ (float)ow, (float)oh }, f, ctx, sv::PictureFilter::Scaler::lanczos, csc);
        floatMatrix.integerMatrix = false;
        auto refused = floatMatrix(randomPicture(sv::PixelFormat::BGRA, iw, ih, 100));
        EXPECT(refused.kind != refused.just);
        // ... and the other direction stays an error
        sv::PictureFilter toBgra({ (float)ow, (float)oh }, sv::PixelFormat::BGRA, ctx, sv::PictureFilter::Scaler::lanczos);
        auto bad = toBgra(randomPicture(f, iw, ih, 100));
        EXPECT(bad.kind != bad.just);
    }
    if (g_fail) std::printf("%d failure(s)\n", g_fail);
    else std::printf("test_lanczos_to_yuv: ok\n");
    return g_fail ? 1 : 0;
}
