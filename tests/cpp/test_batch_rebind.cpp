// tests/cpp/test_batch_rebind.cpp — the C++ host mirror's use of chv_batch_rebind (swiftvideo_amd/host/swiftvideo_hip.hpp): a VideoMixerGroup
// that keeps its batches (reuseBatches) and rebinds them to every tick's pictures gives, tick by tick over rotating rings, the bytes of the
// default group, which builds a batch per tick; a scene change in the middle builds afresh.  Built and run by tests/test_cpp_batch_rebind.py.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

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
    std::vector<std::unique_ptr<sv::VideoMixer>> kept, plain;
    sv::PixelFormat fmts[3] = { sv::PixelFormat::nv12, sv::PixelFormat::BGRA, sv::PixelFormat::BGRA };
    for (int k = 0; k < 3; k++) for (auto *dest : { &kept, &plain })
        dest->emplace_back(new sv::VideoMixer("ws", { 80, 44 }, fmts[k], ctx, "mixer" + std::to_string(k)));
    sv::VideoMixerGroup reusing({ kept[0].get(), kept[1].get(), kept[2].get() }, true);
    sv::VideoMixerGroup building({ plain[0].get(), plain[1].get(), plain[2].get() });
    for (int tick = 0; tick < 13; tick++) {
        const float lw = tick < 7 ? 30.f : 36.f;                     // the scene changes at tick 7: the logo grows
        for (int k = 0; k < 3; k++) for (auto *dest : { &kept, &plain }) {
            sv::PictureSample s = randomPicture(sv::PixelFormat::nv12, 48, 30, 1000 + 10 * tick + k);
            s.matrix = sv::Matrix4::ortho(80, 44) * sv::Matrix4::scale(80, 44); s.borderMatrix = s.matrix; s.revision = "cam";
            (*dest)[(size_t)k]->push(sv::uploadComputePicture(ctx, s));
            sv::PictureSample o = randomPicture(sv::PixelFormat::BGRA, 20, 16, 2000 + 10 * tick + k);
            o.matrix = sv::Matrix4::ortho(80, 44) * sv::Matrix4::translation(8, 6) * sv::Matrix4::scale(lw, 20); o.borderMatrix = o.matrix;
            o.opacity = 0.7f; o.zIndex = 1; o.revision = "logo";
            (*dest)[(size_t)k]->push(sv::uploadComputePicture(ctx, o));
        }
        auto outs = reusing.mix(0.0), refs = building.mix(0.0);
        EXPECT(outs.size() == 3 && refs.size() == 3);
        for (int k = 0; k < 3; k++) {
            EXPECT(outs[(size_t)k].kind == outs[(size_t)k].just && refs[(size_t)k].kind == refs[(size_t)k].just);
            if (outs[(size_t)k].kind == outs[(size_t)k].just && refs[(size_t)k].kind == refs[(size_t)k].just)
                EXPECT(samePlanes(sv::downloadComputePicture(ctx, outs[(size_t)k].value, true), sv::downloadComputePicture(ctx, refs[(size_t)k].value, true)));
        }
    }
    // two canvas formats: built at tick 0 and at tick 7, rebound at the eleven others
    EXPECT(reusing.rebuilds == 4 && reusing.rebinds == 22);
    EXPECT(building.rebuilds == 0 && building.rebinds == 0);
    if (g_fail) std::printf("%d failure(s); %d rebuilds, %d rebinds\n", g_fail, reusing.rebuilds, reusing.rebinds);
    else std::printf("test_batch_rebind: ok\n");
    return g_fail ? 1 : 0;
}
