// tests/cpp/test_stream_select.cpp — stream_select.h on the CPU: which launches of tick_bgra_stream take the opaque-bottom kernels.
// Built and run by tests/test_stream_opaque_select.py; exit status 0 = every expectation held, else the number of the first that did not.
#include "stream_select.h"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace chv;

struct Batch {
    std::vector<DTick> ticks;
    std::vector<DLayer> layers;
    void tick(std::initializer_list<float> opacities) {
        DTick t{};
        t.n_layers = (int)opacities.size();
        t.first_layer = (int)layers.size();
        t.clear_first = 1;
        ticks.push_back(t);
        for (float op : opacities) {
            DLayer l{};
            l.u[U_OPACITY] = op;
            layers.push_back(l);
        }
    }
    bool opaque(int enabled = 1) const { return stream_opaque_bottom(ticks.data(), layers.data(), (int)ticks.size(), enabled); }
};

int main() {
    int n = 0;
#define EXPECT(cond) do { n++; if (!(cond)) { fprintf(stderr, "expectation %d failed: %s\n", n, #cond); return n; } } while (0)
    const float below = std::nextafterf(1.0f, 0.0f), above = std::nextafterf(1.0f, 2.0f);
    EXPECT(below == 0.99999994f);
    { Batch b; b.tick({1.0f, 0.75f, 0.5f, 0.25f}); EXPECT(b.opaque()); EXPECT(!b.opaque(0)); }          // the headline's tick; the switch off
    { Batch b; b.tick({1.0f, 0.0f}); EXPECT(b.opaque()); }                                              // two layers are enough
    { Batch b; b.tick({1.0f, 1.0f, 1.0f}); EXPECT(b.opaque()); }
    { Batch b; b.tick({below, 0.75f}); EXPECT(!b.opaque()); }                                           // 0.99999994f is not 1
    { Batch b; b.tick({above, 0.75f}); EXPECT(!b.opaque()); }
    { Batch b; b.tick({0.0f, 1.0f}); EXPECT(!b.opaque()); }                                             // an opaque UPPER layer does not count
    { Batch b; b.tick({-1.0f, 0.5f}); EXPECT(!b.opaque()); }
    { Batch b; b.tick({NAN, 0.5f}); EXPECT(!b.opaque()); }
    { Batch b; b.tick({1.0f}); EXPECT(!b.opaque()); }                                                   // a one-layer tick has no layer 1 to take the code
    { Batch b; for (int i = 0; i < 5; i++) b.tick({1.0f, 0.1f * i, 0.3f}); EXPECT(b.opaque()); EXPECT(!b.opaque(0)); }
    for (int odd = 0; odd < 5; odd++) {                                                                 // one tick of the batch differs: nobody goes
        Batch b;
        for (int i = 0; i < 5; i++) b.tick({i == odd ? below : 1.0f, 0.5f, 0.3f});
        EXPECT(!b.opaque());
    }
    { Batch b; b.tick({1.0f, 0.5f}); b.tick({1.0f}); EXPECT(!b.opaque()); }
    { Batch b; EXPECT(!b.opaque()); }                                                                   // no ticks
    return 0;
}
