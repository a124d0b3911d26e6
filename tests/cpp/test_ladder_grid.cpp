// test_ladder_grid.cpp — the grid of a Lanczos ladder launch on the CPU (swiftvideo_amd/csrc/lanczos_ladder_grid.h): ladder_order plans as the
// launchers ask it to, and every block of the grid is walked with the scan and the numbering the kernels run.  g++ only, no HIP.
//
// Per case (1 .. 8 rungs, pad 8 as the strip route has it and pad 1 as the tile route): every (rung, item) is the work of exactly one live
// block, the dead blocks are the grid minus the sum of the totals, every range starts on a multiple of pad, first[0] == 0, first[k] ==
// INT_MAX beyond the last rung, totals descend along the launch order and ties keep the caller's order, rung[k].first_block == first[k].
// One case is not walked: a grid beyond 30 bits is refused.
#include "lanczos_ladder_grid.h"

#include <cstdio>
#include <vector>

using namespace chv;

namespace {

// a pending rung as the 4:2:0 units have it: the record, and behind it what the copy carries along (here: the caller's index)
struct Pending {
    LadderRung420 R;
    int caller;
};
struct Args {
    int32_t first[kLanczosPlanarLadderMaxRungs];
    LadderRung420 rung[kLanczosPlanarLadderMaxRungs];
    int caller[kLanczosPlanarLadderMaxRungs];
};

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
                                                                      std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

bool order(Args *a, const std::vector<int> &totals, int pad, unsigned *grid) {
    Pending rungs[kLanczosPlanarLadderMaxRungs] = {};
    for (size_t k = 0; k < totals.size(); k++) {
        rungs[k].R.total = totals[k];
        rungs[k].R.first_block = -1;                               // (the order assigns it)
        rungs[k].caller = (int)k;
    }
    for (int k = 0; k < kLanczosPlanarLadderMaxRungs; k++) a->first[k] = 0;      // (the order must overwrite all of it)
    return ladder_order(a, rungs, (int)totals.size(), pad, grid, [](const Pending &P) { return P.R.total; },
                        [](Args *to, int k, const Pending &P) { to->rung[k] = P.R; to->caller[k] = P.caller; });
}

template <bool XCD>
void walk(const std::vector<int> &totals, int pad, int tag) {
    const int n = (int)totals.size();
    Args a;
    unsigned grid = 0;
    CHECK(order(&a, totals, pad, &grid), "case %d: refused", tag);
    long sum = 0;
    for (int t : totals) sum += t;
    // the plan
    CHECK(a.first[0] == 0, "case %d: first[0] = %d", tag, a.first[0]);
    long at = 0;
    for (int k = 0; k < kLanczosPlanarLadderMaxRungs; k++) {
        if (k >= n) { CHECK(a.first[k] == INT_MAX, "case %d: first[%d] = %d beyond the last rung", tag, k, a.first[k]); continue; }
        CHECK(a.first[k] % pad == 0, "case %d: first[%d] = %d, pad %d", tag, k, a.first[k], pad);
        CHECK(a.first[k] == at, "case %d: first[%d] = %d, the ranges before it end at %ld", tag, k, a.first[k], at);
        CHECK(a.rung[k].first_block == a.first[k], "case %d: rung[%d].first_block = %d, first = %d", tag, k, a.rung[k].first_block, a.first[k]);
        CHECK(a.rung[k].total == totals[a.caller[k]], "case %d: rung[%d] is not the caller's rung %d", tag, k, a.caller[k]);
        if (k) {
            CHECK(a.rung[k - 1].total >= a.rung[k].total, "case %d: totals %d then %d", tag, a.rung[k - 1].total, a.rung[k].total);
            CHECK(a.rung[k - 1].total > a.rung[k].total || a.caller[k - 1] < a.caller[k], "case %d: equal totals, the caller's rungs %d then %d", tag,
                  a.caller[k - 1], a.caller[k]);
        }
        at += ((long)a.rung[k].total + pad - 1) / pad * pad;
    }
    CHECK((long)grid == at, "case %d: grid %u, the ranges end at %ld", tag, grid, at);
    // every block, as a kernel sees it
    std::vector<std::vector<int>> seen(n);
    for (int k = 0; k < n; k++) seen[k].assign(a.rung[k].total, 0);
    long dead = 0;
    for (unsigned b = 0; b < grid; b++) {
        const int r = ladder_rung_of(a.first, (int)b);
        if (r < 0 || r >= n) { CHECK(false, "case %d: block %u in rung %d of %d", tag, b, r, n); continue; }
        const LadderItem it = ladder_item<XCD>((int)b - a.rung[r].first_block, a.rung[r].total);
        if (!it.live) { dead++; continue; }
        if (it.idx < 0 || it.idx >= a.rung[r].total) { CHECK(false, "case %d: block %u: item %d of %d", tag, b, it.idx, a.rung[r].total); continue; }
        seen[r][it.idx]++;
    }
    for (int k = 0; k < n; k++)
        for (int i = 0; i < a.rung[k].total; i++) CHECK(seen[k][i] == 1, "case %d: rung %d item %d is the work of %d blocks", tag, k, i, seen[k][i]);
    CHECK(dead == (long)grid - sum, "case %d: %ld dead blocks, grid %u, work %ld", tag, dead, grid, sum);
}

}  // namespace

int main() {
    const std::vector<std::vector<int>> cases = {
        { 1 }, { 7 }, { 8 }, { 9 }, { 63 }, { 64 }, { 65 }, { 4099 },
        { 1, 7 }, { 9, 9 }, { 8, 65, 8 }, { 63, 64, 65 }, { 7, 3000, 7, 1 },
        { 65, 1, 65, 1, 65 }, { 9, 9, 9, 9, 9, 9 }, { 1, 7, 8, 9, 63, 64, 65 },
        { 1, 7, 8, 9, 63, 64, 65, 5000 }, { 5000, 65, 64, 63, 9, 8, 7, 1 }, { 64, 2047, 64, 9, 2047, 1, 9, 64 }, { 1, 1, 1, 1, 1, 1, 1, 1 },
    };
    int tag = 0;
    for (const auto &c : cases) {
        walk<true>(c, 8, tag++);        // the strip route: ranges padded to the eight XCDs, numbered per XCD
        walk<false>(c, 1, tag++);       // the tile route
    }
    // a grid beyond 30 bits
    Args a;
    unsigned grid = 0;
    CHECK(!order(&a, { 0x20000000, 0x20000000, 0x20000000 }, 8, &grid), "three rungs of 2^29 blocks were not refused");
    CHECK(!order(&a, { 0x20000000, 0x20000000, 0x20000000 }, 1, &grid), "three rungs of 2^29 blocks were not refused (pad 1)");
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
