// tests/cpp/test_f32_taps.cpp — the arithmetic identity behind tick_bgra_stream_cd (cs_mix_d and yuv_to_bgr_fixed_absorbed_d, pixel_math.hip.h) on
// the CPU, bit for bit: with the byte's raw bits B = b x 2^-149 as the sample and 2^127 on the column weight,
//     fma(chain of W x B, 2^22, m)   ==   (w00 t00, three fmaf) + m
// for the weights stream_body forms (column fraction x row fraction, each with its complement), every byte in every tap position and the nine
// conversion constants of the absorbed matrices.  Built and run by tests/test_cpp_f32_taps.py; prints the mismatch count, exit status 0 = none.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

static float bits_to_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t float_to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// my / mu / mv of kCscAbsorbed (pixel_math.hip.h): BT.601 limited, BT.709 limited, BT.709 full
static const float kM[9] = { 10041594.0f, 13672062.0f, 9933686.0f, 8659076.0f, 15468090.0f, 11137308.0f, 8400986.0f, -15564928.0f, -9977984.0f };
static const float kScaleD = 0x1p127f, kUnscaleD = 0x1p22f;

static unsigned long long g_checked = 0, g_bad = 0;

// one (column fraction, row fraction) pair and four bytes, all nine constants
static void check(float a, float b, const uint32_t t[4]) {
    const float ib = 1.0f - b;
    // the reference: weights and chain of cs_mix on converted floats
    const float ia = 1.0f - a;
    const float w00 = ia * ib, w10 = a * ib, w01 = ia * b, w11 = a * b;
    const float r = fmaf(w11, (float)t[3], fmaf(w01, (float)t[2], fmaf(w10, (float)t[1], w00 * (float)t[0])));
    // the f32-tap form: 2^127 on the column weights, raw bits as samples, the chain of cs_mix_d
    const float iaS = (1.0f - a) * kScaleD, aS = a * kScaleD;
    const float W00 = iaS * ib, W10 = aS * ib, W01 = iaS * b, W11 = aS * b;
    const float S = fmaf(W11, bits_to_float(t[3]), fmaf(W01, bits_to_float(t[2]), fmaf(W10, bits_to_float(t[1]), fmaf(W00, bits_to_float(t[0]), 0.0f))));
    for (int k = 0; k < 9; k++) {
        const uint32_t want = float_to_bits(r + kM[k]), got = float_to_bits(fmaf(S, kUnscaleD, kM[k]));
        g_checked++;
        if (want != got) {
            if (g_bad++ < 8) fprintf(stderr, "a=%a b=%a taps %u %u %u %u m=%a: %08x != %08x\n", a, b, t[0], t[1], t[2], t[3], kM[k], got, want);
        }
    }
}

int main() {
    // the denormal operands must be honoured here as on the device
    if (bits_to_float(1u) * 0x1p127f != 0x1p-22f) { fprintf(stderr, "this build flushes denormals\n"); return 2; }
    const float grid[8] = { 0.0f, 0x1p-24f, 0x1p-23f, 0.25f, 1.0f / 3.0f, 0.5f, 1.0f - 0x1p-24f, 1.0f };
    for (float a : grid)
        for (float b : grid)
            for (int pos = 0; pos < 4; pos++)
                for (uint32_t others : { 0u, 255u })
                    for (uint32_t v = 0; v < 256; v++) {
                        uint32_t t[4] = { others, others, others, others };
                        t[pos] = v;
                        check(a, b, t);
                    }
    std::mt19937 rng(20260118u);
    std::uniform_real_distribution<float> frac(0.0f, 1.0f);
    for (int i = 0; i < 1000000; i++) {
        // (fractions as the kernels see them: any float in [0, 1); every eighth pair snapped to the 2^-24 grid of a coordinate past 1)
        float a = frac(rng), b = frac(rng);
        if ((i & 7) == 7) { a = floorf(a * 0x1p24f) * 0x1p-24f; b = floorf(b * 0x1p24f) * 0x1p-24f; }
        const uint32_t w = rng();
        const uint32_t t[4] = { w & 255u, (w >> 8) & 255u, (w >> 16) & 255u, w >> 24 };
        check(a, b, t);
    }
    printf("test_f32_taps: %llu checked, %llu mismatches\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
