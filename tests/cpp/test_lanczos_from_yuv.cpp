// tests/cpp/test_lanczos_from_yuv.cpp — the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) resizing nv12 and y420p pictures into BGRA
// and RGBA planes with Lanczos-3 (scaleLanczosFromYuv): a list of three pictures in one launch == the same three conversions one by one; at
// equal sizes a picture with neutral chroma comes out as the grey section 4.2 makes of its luma bytes, worked out here; an RGBA target holds a
// BGRA target's bytes with red and blue exchanged; PictureFilter takes the pair only with convertToRgb set; a BGRA source and a mixed list are
// errors that launch nothing.  Built and run by tests/test_cpp_lanczos_from_yuv.py.
#include <algorithm>
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
static const uint8_t *pixel(const sv::PictureSample &s, int x, int y) { return s.img->buffers[0]->data() + (size_t)y * s.img->planes[0].stride + (size_t)4 * x; }
static unsigned long long launches() {
    unsigned long long v = 0;
    if (chv_debug_get_counter("lanczos_from_yuv_launches", &v)) g_fail++;
    return v;
}

int main() {
    sv::ComputeContext ctx = sv::makeComputeContext(sv::ComputeDeviceType::GPU);
    const int iw = 192, ih = 108, ow = 128, oh = 72, n = 3;
    // yoff and cy of BT.601 limited, BT.709 limited, BT.601 full, BT.709 full
    const int yoff[4] = { 16, 16, 0, 0 }, cy[4] = { 76309, 76309, 65536, 65536 };
    for (sv::PixelFormat f : { sv::PixelFormat::nv12, sv::PixelFormat::y420p }) {
        std::vector<sv::PictureSample> srcs;
        std::vector<std::pair<sv::PictureSample, sv::PictureSample>> list;
        std::vector<sv::PictureSample> singles;
        for (int i = 0; i < n; i++) {
            srcs.push_back(sv::uploadComputePicture(ctx, randomPicture(f, iw, ih, 100 + i)));
            list.emplace_back(sv::uploadComputePicture(ctx, randomPicture(sv::PixelFormat::BGRA, ow, oh, 300 + i)), srcs.back());
            singles.push_back(sv::uploadComputePicture(ctx, randomPicture(sv::PixelFormat::BGRA, ow, oh, 200 + i)));
        }
        unsigned long long before = launches();
        for (int i = 0; i < n; i++) {
            const sv::PictureSample &d = singles[(size_t)i], &s = srcs[(size_t)i];
            ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosFromYuv(c, d, s, CHV_CSC_BT709_LIMITED); });
        }
        EXPECT(launches() - before == 3);
        before = launches();
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosFromYuv(c, list, CHV_CSC_BT709_LIMITED); });
        EXPECT(launches() - before == 1);
        for (int i = 0; i < n; i++) {
            sv::PictureSample one = sv::downloadComputePicture(ctx, singles[(size_t)i], true), many = sv::downloadComputePicture(ctx, list[(size_t)i].first, true);
            EXPECT(samePlanes(one, many));
            EXPECT(!samePlanes(many, randomPicture(sv::PixelFormat::BGRA, ow, oh, 300 + i)));                    // (the list wrote the target)
        }
        // an RGBA target: the BGRA target's bytes with red and blue exchanged
        sv::PictureSample rgba = sv::uploadComputePicture(ctx, randomPicture(sv::PixelFormat::RGBA, ow, oh, 400));
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosFromYuv(c, rgba, srcs[0], CHV_CSC_BT709_LIMITED); });
        {
            sv::PictureSample a = sv::downloadComputePicture(ctx, rgba, true), b = sv::downloadComputePicture(ctx, singles[0], true);
            bool swapped = true;
            for (int y = 0; y < oh; y++)
                for (int x = 0; x < ow; x++) {
                    const uint8_t *p = pixel(a, x, y), *q = pixel(b, x, y);
                    swapped = swapped && p[0] == q[2] && p[1] == q[1] && p[2] == q[0] && p[3] == 255 && q[3] == 255;
                }
            EXPECT(swapped);
        }
        // at equal sizes the codes pass through (6 taps, the off-centre weights round away): with neutral chroma every pixel is the grey
        // section 4.2 makes of its luma byte, in all four colourspaces — through the call, and through PictureFilter with convertToRgb
        sv::PictureSample host = randomPicture(f, iw, ih, 100);
        for (size_t i = 1; i < host.img->buffers.size(); i++) std::fill(host.img->buffers[i]->begin(), host.img->buffers[i]->end(), (uint8_t)128);
        sv::PictureSample grey = sv::uploadComputePicture(ctx, host);
        for (int csc = 0; csc < 4; csc++) {
            sv::PictureSample same = sv::uploadComputePicture(ctx, randomPicture(sv::PixelFormat::BGRA, iw, ih, 500));
            ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosFromYuv(c, same, grey, csc); });
            sv::PictureFilter filter({ (float)iw, (float)ih }, sv::PixelFormat::BGRA, ctx, sv::PictureFilter::Scaler::lanczos, csc);
            EXPECT(filter(grey).kind != sv::EventBox<sv::PictureSample>::just);                                   // (off by default: the error it always was)
            filter.convertToRgb = true;
            sv::EventBox<sv::PictureSample> out = filter(grey);
            EXPECT(out.kind == sv::EventBox<sv::PictureSample>::just);
            std::vector<sv::PictureSample> got{ sv::downloadComputePicture(ctx, same, true) };
            if (out.kind == sv::EventBox<sv::PictureSample>::just) got.push_back(sv::downloadComputePicture(ctx, out.value, true));
            for (const sv::PictureSample &g : got) {
                bool ok = true;
                for (int y = 0; y < ih; y++)
                    for (int x = 0; x < iw; x++) {
                        const int Y = host.img->buffers[0]->data()[(size_t)y * host.img->planes[0].stride + x];
                        const int v = std::min(std::max((cy[csc] * (Y - yoff[csc]) + 32768) >> 16, 0), 255);
                        const uint8_t *p = pixel(g, x, y);
                        ok = ok && p[0] == v && p[1] == v && p[2] == v && p[3] == 255;
                    }
                EXPECT(ok);
            }
        }
        // an empty list is a no-op; a BGRA source and a list of two target orders are errors that launch nothing
        before = launches();
        ctx = sv::usingContext(ctx, [&](sv::ComputeContext c) { return sv::scaleLanczosFromYuv(c, std::vector<std::pair<sv::PictureSample, sv::PictureSample>>{}); });
        bool threw = false;
        try { sv::scaleLanczosFromYuv(ctx, singles[0], singles[1]); } catch (const sv::ComputeError &) { threw = true; }
        EXPECT(threw);
        threw = false;
        try { sv::scaleLanczosFromYuv(ctx, srcs[0], srcs[1]); } catch (const sv::ComputeError &) { threw = true; }       // an nv12 / y420p target
        EXPECT(threw);
        std::vector<std::pair<sv::PictureSample, sv::PictureSample>> mixed{ list[0], { rgba, srcs[1] } };
        threw = false;
        try { sv::scaleLanczosFromYuv(ctx, mixed); } catch (const sv::ComputeError &) { threw = true; }
        EXPECT(threw);
        EXPECT(launches() == before);
    }
    if (g_fail) std::printf("%d failure(s)\n", g_fail);
    else std::printf("test_lanczos_from_yuv: ok\n");
    return g_fail ? 1 : 0;
}
