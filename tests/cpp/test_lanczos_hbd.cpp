// tests/cpp/test_lanczos_hbd.cpp — the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) taking 10-bit decoder frames (decoderFramePlanes:
// p010, y420p10) into nv12 and y420p pictures with Lanczos-3 (scaleLanczosHbdTo420): a ladder of three rungs of two pictures == the same six
// calls one by one, in as many launches as the rungs take routes; at equal sizes every luma byte is min(rint(code / 4), 255) of the sample at
// its place, whatever the ignored bits hold; PictureFilter takes the pair only with convertHighBitDepth set; an 8-bit source, an odd pitch and
// nine rungs are errors that launch nothing.  Built and run by tests/test_cpp_lanczos_hbd.py.
#include <cmath>
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
// a decoder frame: the planes decoderFramePlanes describes, rows of `stride` bytes — every bit seeded, the ignored ones included
static sv::PictureSample decoderFrame(sv::PixelFormat f, int w, int h, uint64_t seed) {
    auto img = std::make_shared<sv::ImageBuffer>();
    img->pixelFormat = f; img->bufferType = sv::BufferType::cpu; img->size = { (float)w, (float)h };
    img->planes = sv::decoderFramePlanes(f, img->size);
    for (size_t i = 0; i < img->planes.size(); i++) {
        img->buffers.push_back(std::make_shared<sv::Data>((size_t)img->planes[i].stride * (size_t)img->planes[i].size.y, 0));
        fill(*img->buffers.back(), seed * 16 + i);
    }
    sv::PictureSample s;
    s.img = img; s.assetId = "dec"; s.borderMatrix = s.matrix;
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
// the byte the specification stores for luma sample (x, y) of a decoder frame at equal sizes
static uint8_t lumaByteOf(const sv::PictureSample &s, int x, int y) {
    const uint8_t *row = s.img->buffers[0]->data() + (size_t)y * s.img->planes[0].stride;
    const unsigned word = row[2 * x] | (unsigned)row[2 * x + 1] << 8;
    const unsigned code = s.pixelFormat() == sv::PixelFormat::p010 ? word >> 6 : word & 1023u;
    return (uint8_t)std::min(std::nearbyint(code / 4.0), 255.0);          // (the default rounding mode: ties to even)
}
static unsigned long long launches() {
    unsigned long long v = 0;
    if (chv_debug_get_counter("lanczos_hbd_launches", &v)) g_fail++;
    return v;
}

int main() {
    sv::ComputeContext ctx = sv::makeComputeContext(sv::ComputeDeviceType::GPU);
    const int iw = 96, ih = 54, n = 2;
    const int sizes[3][2] = { { 80, 46 }, { 64, 36 }, { 16, 10 } };        // the last one: 6:1, 36 taps — the tile route
    for (sv::PixelFormat f : { sv::PixelFormat::p010, sv::PixelFormat::y420p10 }) {
        for (sv::PixelFormat g : { sv::PixelFormat::nv12, sv::PixelFormat::y420p }) {
            std::vector<sv::PictureSample> srcs;
            std::vector<std::vector<sv::PictureSample>> rungs(3), singles(3);
            for (int i = 0; i < n; i++) srcs.push_back(sv::uploadComputePicture(ctx, decoderFrame(f, iw, ih, 100 + i)));
            for (int r = 0; r < 3; r++)
                for (int i = 0; i < n; i++) {
                    rungs[(size_t)r].push_back(sv::uploadComputePicture(ctx, randomPicture(g, sizes[r][0], sizes[r][1], 300 + 8 * r + i)));
                    singles[(size_t)r].push_back(sv::uploadComputePicture(ctx, randomPicture(g, sizes[r][0], sizes[r][1], 200 + 8 * r + i)));
                }
            unsigned long long before = launches();
            for (int r = 0; r < 3; r++)
                for (int i = 0; i < n; i++) {
                    const sv::PictureSample &d = singles[(size_t)r][(size_t)i], &s = srcs[(size_t)i];
                    ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosHbdTo420(c, d, s); });
                }
            EXPECT(launches() - before == 6);
            before = launches();
            ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosHbdTo420(c, rungs, srcs); });
            EXPECT(launches() - before == 2);
            for (int r = 0; r < 3; r++)
                for (int i = 0; i < n; i++) {
                    sv::PictureSample one = sv::downloadComputePicture(ctx, singles[(size_t)r][(size_t)i], true), many = sv::downloadComputePicture(ctx, rungs[(size_t)r][(size_t)i], true);
                    EXPECT(samePlanes(one, many));
                    EXPECT(!samePlanes(many, randomPicture(g, sizes[r][0], sizes[r][1], 300 + 8 * r + i)));          // (the ladder wrote the target)
                }
            // at equal sizes Y is the code over four, through the call and through PictureFilter with convertHighBitDepth
            sv::PictureSample host = decoderFrame(f, iw, ih, 100);
            sv::PictureSample same = sv::uploadComputePicture(ctx, randomPicture(g, iw, ih, 500));
            ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosHbdTo420(c, same, srcs[0]); });
            sv::PictureFilter filter({ (float)iw, (float)ih }, g, ctx, sv::PictureFilter::Scaler::lanczos);
            EXPECT(filter(srcs[0]).kind != sv::EventBox<sv::PictureSample>::just);                                    // (off by default: the error it always was)
            filter.convertDecoderFormats = true;
            EXPECT(filter(srcs[0]).kind != sv::EventBox<sv::PictureSample>::just);                                    // (the 8-bit flag does not open it)
            filter.convertHighBitDepth = true;
            sv::EventBox<sv::PictureSample> out = filter(host);                                                       // (a CPU frame: uploaded first)
            EXPECT(out.kind == sv::EventBox<sv::PictureSample>::just);
            sv::PictureSample a = sv::downloadComputePicture(ctx, same, true);
            bool luma = true;
            for (int y = 0; y < ih; y++)
                for (int x = 0; x < iw; x++) luma = luma && a.img->buffers[0]->data()[(size_t)y * a.img->planes[0].stride + x] == lumaByteOf(host, x, y);
            EXPECT(luma);
            if (out.kind == sv::EventBox<sv::PictureSample>::just) EXPECT(samePlanes(sv::downloadComputePicture(ctx, out.value, true), a));
            // an empty ladder is a no-op; an 8-bit source, an odd pitch and nine rungs are errors that launch nothing
            before = launches();
            ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosHbdTo420(c, std::vector<std::vector<sv::PictureSample>>{}, std::vector<sv::PictureSample>{}); });
            bool threw = false;
            sv::PictureSample eight = sv::uploadComputePicture(ctx, randomPicture(sv::PixelFormat::nv12, iw, ih, 600));
            try { sv::scaleLanczosHbdTo420(ctx, singles[0][0], eight); } catch (const sv::ComputeError &) { threw = true; }
            EXPECT(threw);
            sv::PictureSample odd = srcs[0];
            odd.img = std::make_shared<sv::ImageBuffer>(*srcs[0].img);
            odd.img->gpuPitches[0] -= 1;
            threw = false;
            try { sv::scaleLanczosHbdTo420(ctx, singles[0][0], odd); } catch (const sv::ComputeError &) { threw = true; }
            EXPECT(threw);
            std::vector<std::vector<sv::PictureSample>> nine;
            for (int r = 0; r < 9; r++) nine.push_back(rungs[(size_t)(r % 3)]);
            threw = false;
            try { sv::scaleLanczosHbdTo420(ctx, nine, srcs); } catch (const sv::ComputeError &) { threw = true; }
            EXPECT(threw);
            EXPECT(launches() == before);
        }
    }
    if (g_fail) std::printf("%d failure(s)\n", g_fail);
    else std::printf("test_lanczos_hbd: ok\n");
    return g_fail ? 1 : 0;
}
