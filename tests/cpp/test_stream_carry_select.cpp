// tests/cpp/test_stream_carry_select.cpp — stream_select.h on the CPU: which opaque-bottom launches of tick_bgra_stream take the chroma-carry
// kernels.  Built and run by tests/test_stream_carry_select.py; exit status 0 = every expectation held, else the number of the first that
// did not.
#include "stream_select.h"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace chv;

struct Batch {
    std::vector<DTick> ticks;
    std::vector<DLayer> layers;
    // a tick of `nl` layers: canvas H rows, a source of `src_h` luma rows (chroma: src_h / 2) drawn over `rect_h` canvas rows
    void tick(int nl, int H, int src_h, double rect_h = 0.0, float tex_scale = 1.0f) {
        DTick t{};
        t.n_layers = nl;
        t.first_layer = (int)layers.size();
        t.clear_first = 1;
        t.W = 320;
        t.H = H;
        ticks.push_back(t);
        for (int l = 0; l < nl; l++) {
            DLayer y{};
            y.u[U_OPACITY] = l ? 0.5f : 1.0f;
            y.u[U_TRANSFORM + 5] = (float)(H / (2.0 * (rect_h > 0.0 ? rect_h : (double)H)));       // the inverse of ortho x scale(rect): H / (2 rect_h)
            y.u[U_TEXTURE + 5] = tex_scale;
            y.src.pl[0].h = src_h;
            y.src.pl[1].h = src_h / 2;
            layers.push_back(y);
        }
    }
    bool carry(bool planar = false, bool by_value = false, int enabled = 1) const {
        return stream_chroma_carry(ticks.data(), layers.data(), (int)ticks.size(), planar, by_value, enabled);
    }
};

int main() {
    int n = 0;
#define EXPECT(cond) do { n++; if (!(cond)) { fprintf(stderr, "expectation %d failed: %s\n", n, #cond); return n; } } while (0)
    { Batch b; b.tick(4, 720, 1080); EXPECT(b.carry()); }                                       // the headline's tick: 540 chroma rows over 720
    { Batch b; b.tick(4, 720, 1080); EXPECT(!b.carry(false, false, 0)); }                       // the switch off
    { Batch b; b.tick(4, 720, 1080); EXPECT(!b.carry(true)); }                                  // planar sources
    { Batch b; b.tick(4, 720, 1080); EXPECT(!b.carry(false, true)); }                           // the by-value lone tick
    { Batch b; b.tick(2, 70, 36); EXPECT(b.carry()); }                                          // an enlargement
    // the boundary: one chroma row per canvas row is taken, the next representable ratio above it is not
    { Batch b; b.tick(3, 52, 104); EXPECT(b.carry()); }
    { Batch b; b.tick(3, 52, 106); EXPECT(!b.carry()); }
    { Batch b; b.tick(3, 51, 104); EXPECT(!b.carry()); }
    { Batch b; b.tick(3, 52, 104, 0.0, std::nextafterf(1.0f, 2.0f)); EXPECT(!b.carry()); }      // (the texture matrix stretches the rows by one ulp)
    { Batch b; b.tick(3, 52, 104, 0.0, std::nextafterf(1.0f, 0.0f)); EXPECT(b.carry()); }
    { Batch b; b.tick(3, 52, 208); EXPECT(!b.carry()); }                                        // two chroma rows per canvas row
    { Batch b; b.tick(2, 33, 130); EXPECT(!b.carry()); }                                        // 4 : 1 down
    // a picture inside the canvas: the ratio is that of the rectangle, not of the canvas
    { Batch b; b.tick(4, 70, 90, 60.0); EXPECT(b.carry()); }                                    // 45 chroma rows over 60 canvas rows
    { Batch b; b.tick(4, 70, 90, 40.0); EXPECT(!b.carry()); }                                   // 45 over 40
    // every tick of a batch has to qualify
    { Batch b; for (int i = 0; i < 4; i++) b.tick(3, 720, 1080); EXPECT(b.carry()); }
    for (int odd = 0; odd < 4; odd++) {
        Batch b;
        for (int i = 0; i < 4; i++) b.tick(3, i == odd ? 200 : 720, 1080);
        EXPECT(!b.carry());
    }
    // what the kernels are not built for
    { Batch b; b.tick(1, 720, 1080); EXPECT(!b.carry()); }
    { Batch b; b.tick(5, 720, 1080); EXPECT(!b.carry()); }
    { Batch b; b.tick(4, 720, 1080, 0.0, -1.0f); EXPECT(!b.carry()); }                          // (a flip never gets here; it must not pass either)
    { Batch b; b.tick(4, 720, 1080, 0.0, NAN); EXPECT(!b.carry()); }
    { Batch b; EXPECT(!b.carry()); }                                                            // no ticks
    return 0;
}
