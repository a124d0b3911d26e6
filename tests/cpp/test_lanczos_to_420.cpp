// tests/cpp/test_lanczos_to_420.cpp — the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) taking decoder frames of the five formats
// planesForFormat does not know (decoderFramePlanes: nv21, y422p, y444p, yuvs, zvuy) into nv12 and y420p pictures with Lanczos-3
// (scaleLanczosTo420): a ladder of three rungs of two pictures == the same six calls one by one, in as many launches as the rungs take
// routes; at equal sizes the luma plane is the source's Y bytes; PictureFilter takes the pair only with convertDecoderFormats set; a BGRA
// source, a packed picture of odd width and nine rungs are errors that launch nothing.  Built and run by tests/test_cpp_lanczos_to_420.py.
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
// a decoder frame: the planes decoderFramePlanes describes, rows of `stride` bytes
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
// Y of pixel (x, y) of a decoder frame
static uint8_t lumaOf(const sv::PictureSample &s, int x, int y) {
    const sv::PixelFormat f = s.pixelFormat();
    const uint8_t *row = s.img->buffers[0]->data() + (size_t)y * s.img->planes[0].stride;
    if (f == sv::PixelFormat::yuvs) return row[2 * x];
    if (f == sv::PixelFormat::zvuy) return row[2 * x + 1];
    return row[x];
}
static unsigned long long launches() {
    unsigned long long v = 0;
    if (chv_debug_get_counter("lanczos_to_420_launches", &v)) g_fail++;
    return v;
}

int main() {
    sv::ComputeContext ctx = sv::makeComputeContext(sv::ComputeDeviceType::GPU);
    const int iw = 96, ih = 54, n = 2;
    const int sizes[3][2] = { { 80, 46 }, { 64, 36 }, { 16, 10 } };        // the last one: 6:1, beyond 22 taps for every source — the tile route
    for (sv::PixelFormat f : { sv::PixelFormat::nv21, sv::PixelFormat::y422p, sv::PixelFormat::y444p, sv::PixelFormat::yuvs, sv::PixelFormat::zvuy }) {
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
                    ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosTo420(c, d, s); });
                }
            EXPECT(launches() - before == 6);
            before = launches();
            ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosTo420(c, rungs, srcs); });
            EXPECT(launches() - before == 2);
            for (int r = 0; r < 3; r++)
                for (int i = 0; i < n; i++) {
                    sv::PictureSample one = sv::downloadComputePicture(ctx, singles[(size_t)r][(size_t)i], true), many = sv::downloadComputePicture(ctx, rungs[(size_t)r][(size_t)i], true);
                    EXPECT(samePlanes(one, many));
                    EXPECT(!samePlanes(many, randomPicture(g, sizes[r][0], sizes[r][1], 300 + 8 * r + i)));          // (the ladder wrote the target)
                }
            // at equal sizes Y is an exact copy or unpack, through the call and through PictureFilter with convertDecoderFormats
            sv::PictureSample host = decoderFrame(f, iw, ih, 100);
            sv::PictureSample same = sv::uploadComputePicture(ctx, randomPicture(g, iw, ih, 500));
            ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosTo420(c, same, srcs[0]); });
            sv::PictureFilter filter({ (float)iw, (float)ih }, g, ctx, sv::PictureFilter::Scaler::lanczos);
            EXPECT(filter(srcs[0]).kind != sv::EventBox<sv::PictureSample>::just);                                    // (off by default: the error it always was)
            filter.convertDecoderFormats = true;
            sv::EventBox<sv::PictureSample> out = filter(host);                                                       // (a CPU frame: uploaded first)
            EXPECT(out.kind == sv::EventBox<sv::PictureSample>::just);
            sv::PictureSample a = sv::downloadComputePicture(ctx, same, true);
            bool luma = true;
            for (int y = 0; y < ih; y++)
                for (int x = 0; x < iw; x++) luma = luma && a.img->buffers[0]->data()[(size_t)y * a.img->planes[0].stride + x] == lumaOf(host, x, y);
            EXPECT(luma);
            if (out.kind == sv::EventBox<sv::PictureSample>::just) EXPECT(samePlanes(sv::downloadComputePicture(ctx, out.value, true), a));
            // an empty ladder is a no-op; a BGRA source, a packed picture of odd width and nine rungs are errors that launch nothing
            before = launches();
            ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosTo420(c, std::vector<std::vector<sv::PictureSample>>{}, std::vector<sv::PictureSample>{}); });
            bool threw = false;
            sv::PictureSample bgra = sv::uploadComputePicture(ctx, randomPicture(sv::PixelFormat::BGRA, iw, ih, 600));
            try { sv::scaleLanczosTo420(ctx, singles[0][0], bgra); } catch (const sv::ComputeError &) { threw = true; }
            EXPECT(threw);
            if (f == sv::PixelFormat::yuvs || f == sv::PixelFormat::zvuy) {
                sv::PictureSample odd = srcs[0];
                odd.img = std::make_shared<sv::ImageBuffer>(*srcs[0].img);
                odd.img->planes[0].size.x -= 1;
                threw = false;
                try { sv::scaleLanczosTo420(ctx, singles[0][0], odd); } catch (const sv::ComputeError &) { threw = true; }
                EXPECT(threw);
            }
            std::vector<std::vector<sv::PictureSample>> nine;
            for (int r = 0; r < 9; r++) nine.push_back(rungs[(size_t)(r % 3)]);
            threw = false;
            try { sv::scaleLanczosTo420(ctx, nine, srcs); } catch (const sv::ComputeError &) { threw = true; }
            EXPECT(threw);
            EXPECT(launches() == before);
        }
    }
    if (g_fail) std::printf("%d failure(s)\n", g_fail);
    else std::printf("test_lanczos_to_420: ok\n");
    return g_fail ? 1 : 0;
}
