// lanczos_ladder_grid.h — the grid of a Lanczos ladder launch, for the host and the device (no HIP in here:
// tests/cpp/test_ladder_grid.cpp walks every block of such grids on the CPU).
//
// A launch carries up to eight rungs.  Its grid is the concatenation of the rungs' block ranges, largest rung first (the grid's tail is made
// of the small rungs' blocks); every range starts on a multiple of `pad` blocks and is padded to one.  first[k] is where rung k's range
// starts, INT_MAX beyond the last rung: a block finds its rung by a scalar scan of first[], then its work inside the rung's range — with the
// XCD-aware numbering run PER RUNG when pad is 8, so that blocks of equal b & 7 still share an XCD and neighbouring blocks of one picture
// of one rung stay on one.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <climits>

#ifndef CHV_HOST_DEVICE
#if defined(__HIPCC__)
#define CHV_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define CHV_HOST_DEVICE inline
#endif
#endif

namespace chv {

constexpr int kLanczosPlanarLadderMaxRungs = 8;

// a rung of the 4:2:0 ladder units (the other units' records carry their own geometry; what they share with this one is first_block and total)
struct LadderRung420 {
    int32_t first_block;              // where the rung's range starts in the grid
    int32_t total, per_picture;       // blocks of all pictures (the range in the grid: `total` rounded up to `pad`), blocks per picture
    int32_t T;                        // strip route: the rung's tap class (6 / 8 / 12 / 16 / 22 over its largest tap count)
    int32_t dst_at;                   // the rung's first target plane within a picture's record
    int32_t pad[3];
};

// the rung whose range holds block b: first[] ascends, first[0] == 0
CHV_HOST_DEVICE int ladder_rung_of(const int32_t *first, int b) {
    int r = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 1; k < kLanczosPlanarLadderMaxRungs; k++) r = b >= first[k] ? k : r;
    return r;
}

// What block b of a rung's range (counted from the rung's first_block) works on: item idx of the rung's `total`, or nothing (live false: the
// padding).  XCD: block b runs on XCD b % 8, and an XCD owns a contiguous run of items.
struct LadderItem {
    int idx;
    bool live;
};
template <bool XCD>
CHV_HOST_DEVICE LadderItem ladder_item(int b, int total) {
    LadderItem o;
    o.idx = b;
    if (XCD) {
        const int per_xcd = (total + 7) >> 3;
        o.idx = (b & 7) * per_xcd + (b >> 3);
        o.live = (b >> 3) < per_xcd && o.idx < total;
    } else {
        o.live = o.idx < total;
    }
    return o;
}

// The records of one launch, largest range first (ties keep the caller's order): total(rungs[i]) is a pending rung's block count,
// copy(a, k, rungs[i]) makes it a->rung[k]; first_block and first[] are assigned here.  *grid: the blocks of the launch.  False when the grid
// would not fit 30 bits.
template <class Args, class Pending, class Total, class Copy>
inline bool ladder_order(Args *a, const Pending *rungs, int n, int pad, unsigned *grid, Total total, Copy copy) {
    int order[kLanczosPlanarLadderMaxRungs];
    for (int k = 0; k < n; k++) order[k] = k;
    std::stable_sort(order, order + n, [&](int x, int y) { return total(rungs[x]) > total(rungs[y]); });
    long first = 0;
    for (int k = 0; k < kLanczosPlanarLadderMaxRungs; k++) a->first[k] = INT_MAX;
    for (int k = 0; k < n; k++) {
        copy(a, k, rungs[order[k]]);
        a->rung[k].first_block = (int32_t)first;
        a->first[k] = (int32_t)first;
        first += ((long)a->rung[k].total + pad - 1) / pad * pad;
        if (first > 0x3fffffff) return false;
    }
    *grid = (unsigned)first;
    return true;
}
// (a pending rung that is its record)
template <class Args, class Rung>
inline bool ladder_order(Args *a, const Rung *rungs, int n, int pad, unsigned *grid) {
    return ladder_order(a, rungs, n, pad, grid, [](const Rung &R) { return R.total; }, [](Args *to, int k, const Rung &R) { to->rung[k] = R; });
}

}  // namespace chv
