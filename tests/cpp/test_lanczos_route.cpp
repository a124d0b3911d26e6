// test_lanczos_route.cpp — the integer rules of the Lanczos units' host halves on the CPU (swiftvideo_amd/csrc/lanczos_route.h): the tap class,
// the rows-per-wave rule, the 160 KB refusal and the strip-route rule.  g++ only, no HIP.
//
// Every table below was printed by the copies these functions replaced (planar_strip_route, x420_strip_route, rgb_strip_class and the lambda
// of fy_strip_route, planar_ / rgb_ / fy_ / to_yuv_strip_rows, planar_ / rgb_ / to_yuv_refuses), compiled side by side and found to agree with
// each other, before they were deleted: the shared functions must go on saying what the units said.
#include "lanczos_route.h"

#include <cmath>
#include <cstdio>

using namespace chv;

namespace {

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
                                                                      std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

// lanczos_host_table's rule (chipvideo.cpp)
int taps(int in, int out) {
    const double scale = (double)in / (double)out, fs = scale > 1.0 ? scale : 1.0;
    return 2 * (int)std::ceil(3.0 * fs);
}

// tap counts 1 .. 23
const int kClass[23] = { 6, 6, 6, 6, 6, 6, 8, 8, 12, 12, 12, 12, 16, 16, 16, 16, 22, 22, 22, 22, 22, 22, 22 };

// (strip, output row) pairs of a launch -> rows per wave with at most 64 (the planar and the 4-component ladder units), at most 32 (from_yuv),
// at most 256 and rounded up to even (to_yuv)
const struct { long work; int most64, most32, even256; } kRows[] = {
    { 0L, 8, 8, 8 },          { 1L, 8, 8, 8 },          { 98304L, 8, 8, 8 },        { 98305L, 9, 9, 10 },
    { 110592L, 9, 9, 10 },    { 380929L, 32, 32, 32 },  { 393216L, 32, 32, 32 },    { 393217L, 33, 32, 34 },
    { 774145L, 64, 32, 64 },  { 786432L, 64, 32, 64 },  { 786433L, 64, 32, 66 },    { 2457600L, 64, 32, 200 },
    { 3121153L, 64, 32, 256 }, { 3133441L, 64, 32, 256 }, { 3145733L, 64, 32, 256 }, { 1099511627776L, 64, 32, 256 },
};

// the refusal for a 24 x 24 target from sources of 1:8 to 30:1 on each axis, tap counts by lanczos_host_table's rule.  Rows: source height,
// columns: source width, both over kSizes; X: refused.
const int kSizes[18] = { 3, 6, 12, 24, 36, 48, 60, 84, 96, 120, 168, 240, 336, 400, 480, 560, 640, 720 };
const char *const kRefuses[18] = {
    "..................", "..................", "..................", "..................", "..................", "..................",
    "..................", "..................", "..................", "..................", "..................", "..................",
    "...............XXX", "..............XXXX", ".............XXXXX", "............XXXXXX", "............XXXXXX", "...........XXXXXXX",
};

// The strip-route rule for one plane 48 texels wide with 6 vertical taps, per source width: route, tap class, the plane's nv and the longest
// ring slot, for the plane pairs (target components <- source components) 1 <- 1, 2 <- 2 (both: planar_strip_route AND x420_strip_route, which
// agreed), 2 <- 1 (two source planes in one slot) and 1 <- 2
const struct { int sw; int v[4][4]; } kRoute[] = {
    { 6,   { { 1, 6, 4, 4 },    { 1, 6, 4, 4 },    { 1, 6, 4, 8 },    { 1, 6, 5, 5 } } },
    { 24,  { { 1, 6, 5, 5 },    { 1, 6, 6, 6 },    { 1, 6, 4, 8 },    { 1, 6, 8, 8 } } },
    { 48,  { { 1, 6, 7, 7 },    { 1, 6, 8, 8 },    { 1, 6, 5, 10 },   { 1, 6, 12, 12 } } },
    { 72,  { { 1, 12, 10, 10 }, { 1, 12, 10, 10 }, { 1, 12, 7, 14 },  { 1, 12, 16, 16 } } },
    { 96,  { { 1, 12, 12, 12 }, { 1, 12, 12, 12 }, { 1, 12, 8, 16 },  { 1, 12, 20, 20 } } },
    { 120, { { 1, 16, 14, 14 }, { 1, 16, 15, 15 }, { 1, 16, 9, 18 },  { 1, 16, 25, 25 } } },
    { 144, { { 1, 22, 16, 16 }, { 1, 22, 17, 17 }, { 1, 22, 10, 20 }, { 1, 22, 29, 29 } } },
    { 160, { { 1, 22, 18, 18 }, { 1, 22, 19, 19 }, { 1, 22, 11, 22 }, { 1, 22, 32, 32 } } },
    { 168, { { 1, 22, 18, 18 }, { 1, 22, 19, 19 }, { 1, 22, 11, 22 }, { 1, 22, 33, 33 } } },
    { 172, { { 1, 22, 19, 19 }, { 1, 22, 20, 20 }, { 1, 22, 11, 22 }, { 1, 22, 34, 34 } } },
    { 176, { { 1, 22, 19, 19 }, { 1, 22, 20, 20 }, { 1, 22, 12, 24 }, { 1, 22, 35, 35 } } },
    { 180, { { 0, 22, 0, 0 },   { 0, 22, 0, 0 },   { 0, 22, 0, 0 },   { 0, 22, 0, 0 } } },      // 24 taps: the tile route, nv untouched
    { 192, { { 0, 22, 0, 0 },   { 0, 22, 0, 0 },   { 0, 22, 0, 0 },   { 0, 22, 0, 0 } } },
    { 240, { { 0, 22, 0, 0 },   { 0, 22, 0, 0 },   { 0, 22, 0, 0 },   { 0, 22, 0, 0 } } },
};
const int kPair[4][2] = { { 1, 1 }, { 2, 2 }, { 2, 1 }, { 1, 2 } };      // OC, SC

PlanarPlane plane(int dw, int sw, int oc, int sc, int tx, int ty) {
    PlanarPlane g = {};
    g.dst = DPlane{ nullptr, dw, 48, 0, oc };
    g.src = DPlane{ nullptr, sw, 48, 0, sc };
    g.tx = tx; g.ty = ty;
    return g;
}

}  // namespace

int main() {
    for (int t = 1; t <= 23; t++) CHECK(lanczos_tap_class(t) == kClass[t - 1], "%d taps: class %d, the units had %d", t, lanczos_tap_class(t), kClass[t - 1]);

    for (const auto &r : kRows) {
        CHECK(lanczos_strip_rows(r.work, 64) == r.most64, "work %ld, at most 64: %d rows, the units had %d", r.work, lanczos_strip_rows(r.work, 64), r.most64);
        CHECK(lanczos_strip_rows(r.work, 32) == r.most32, "work %ld, at most 32: %d rows, the unit had %d", r.work, lanczos_strip_rows(r.work, 32), r.most32);
        const int even = (lanczos_strip_rows(r.work, 256) + 1) & ~1;        // (to_yuv_strip_rows)
        CHECK(even == r.even256, "work %ld, at most 256 and even: %d rows, the unit had %d", r.work, even, r.even256);
    }

    for (int i = 0; i < 18; i++)
        for (int j = 0; j < 18; j++) {
            const int sh = kSizes[i], sw = kSizes[j];
            const bool got = lanczos_refuses(24, 24, sw, sh, taps(sw, 24), taps(sh, 24));
            CHECK(got == (kRefuses[i][j] == 'X'), "%d x %d -> 24 x 24: refused %d", sw, sh, (int)got);
        }
    // the bound itself: 160 rows x (32 + 224 columns) x 4 bytes IS 160 KB and passes; one row or one vector of columns more does not
    CHECK(!lanczos_refuses(1, 1, 26, 40, 40, 38), "exactly 160 KB was refused");
    CHECK(lanczos_refuses(1, 1, 26, 40, 40, 39), "161 rows were not refused");
    CHECK(lanczos_refuses(1, 1, 26, 40, 44, 38), "228 columns were not refused");

    for (const auto &r : kRoute)
        for (int pair = 0; pair < 4; pair++) {
            const int oc = kPair[pair][0], sc = kPair[pair][1], *want = r.v[pair];
            PlanarPlane g = plane(48, r.sw, oc, sc, taps(r.sw, 48), 6);
            int T = -1, ring = -1;
            const bool strip = x420_strip_route(&g, 1, &T, &ring);
            CHECK(strip == (want[0] != 0) && T == want[1] && g.nv == want[2] && ring == want[3],
                  "%d <- %d components, %d -> 48: route %d class %d nv %d ring %d, the units had %d %d %d %d", oc, sc, r.sw, (int)strip, T, g.nv, ring, want[0],
                  want[1], want[2], want[3]);
        }

    // the rule's two bounds, with tap counts no table has: a ring slot of exactly 64 vectors is a strip, 66 are not, nor are 23 taps
    {
        const struct { int sw, tx, strip, nv, ring; } edge[] = { { 355, 22, 1, 64, 64 }, { 368, 22, 0, 66, 66 }, { 355, 23, 0, 0, 0 }, { 48, 23, 0, 0, 0 } };
        for (const auto &e : edge) {
            PlanarPlane g = plane(48, e.sw, 1, 2, e.tx, 6);
            int T = -1, ring = -1;
            const bool strip = x420_strip_route(&g, 1, &T, &ring);
            CHECK(strip == (e.strip != 0) && T == 22 && g.nv == e.nv && ring == e.ring, "1 <- 2 components, %d -> 48, %d taps: route %d class %d nv %d ring %d",
                  e.sw, e.tx, (int)strip, T, g.nv, ring);
        }
    }

    // planar_strip_route IS x420_strip_route on same-format geometries: both planes of an NV12 picture and all three of a y420p one, every
    // scale of the sweep on the horizontal axis, a few on the vertical (its tap count alone enters the rule)
    for (int sw : kSizes)
        for (int sh : { 12, 48, 100, 180 })
            for (int np = 2; np <= 3; np++) {
                PlanarPlane a[3], b[3];
                for (int p = 0; p < np; p++) {
                    const int c = np == 2 && p == 1 ? 2 : 1, dw = p ? 24 : 48, w = p ? (sw + 1) / 2 : sw, h = p ? (sh + 1) / 2 : sh;
                    a[p] = b[p] = plane(dw, w, c, c, taps(w, dw), taps(h, p ? 24 : 48));
                }
                int Ta = -1, Tb = -2, ra = -1, rb = -2;
                const bool sa = planar_strip_route(a, np, &Ta, &ra), sb = x420_strip_route(b, np, &Tb, &rb);
                CHECK(sa == sb && Ta == Tb && ra == rb, "%d x %d, %d planes: planar %d %d %d, x420 %d %d %d", sw, sh, np, (int)sa, Ta, ra, (int)sb, Tb, rb);
                for (int p = 0; p < np; p++) CHECK(a[p].nv == b[p].nv, "%d x %d, plane %d of %d: nv %d and %d", sw, sh, p, np, a[p].nv, b[p].nv);
            }

    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
