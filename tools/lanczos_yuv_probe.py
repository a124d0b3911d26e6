"""tools/lanczos_yuv_probe.py [--n 64] [--runs 30] [--out file.json] — device time of chv_scale_lanczos_batch for batches of n pictures at
1920x1080 -> 1280x720 and 3840x2160 -> 1920x1080 (and, recorded only, 1366x768 -> 854x480, whose rows are not whole 16-byte vectors) in three formats: BGRA (the 4-component kernels), nv12 and y420p (the planar kernels), in ONE
process on one device, the formats alternating run by run.  chv_event_* around each batch, warm-up first, the median of `runs` timed runs per
case; then one lone picture of each (chv_scale_lanczos + the host wait, wall time).  Prints a table with the algorithmic GB/s (source + target
payload bytes over time), the share of the 8 TB/s peak and the ratio to BGRA, and the line "condition: ok" when nv12 <= BGRA and y420p <= BGRA
at the two sizes of the condition.  Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import gpuutil as G          # noqa: E402
import util                  # noqa: E402
from swiftvideo_amd import chipvideo as cv       # noqa: E402
from swiftvideo_amd import compute as sv         # noqa: E402

PEAK = 8.0e12
SIZES = [(1920, 1080, 1280, 720), (3840, 2160, 1920, 1080)]
# recorded, not part of the condition: rows that are NOT whole 16-byte vectors (1366 luma bytes, 1366 CbCr bytes, 683 Cb / Cr bytes) — the planar
# strip kernel's compiler-managed loads and byte gather instead of its hand-awaited vector loads
UNALIGNED_SIZES = [(1366, 768, 854, 480)]
FORMATS = ["bgra", "nv12", "y420p"]


def payload_bytes(fmt, w, h):
    return sum(max(r, 1) * max(c, 1) * comps for r, c, comps in util.plane_shapes(fmt, w, h))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = cv.load()
    ctx = sv.makeComputeContext(forType="GPU")

    def event():
        h = C.c_void_p()
        cv.check(lib.chv_event_create(ctx.handle, C.byref(h)))
        return h
    e0, e1 = event(), event()
    results = []
    for iw, ih, ow, oh in SIZES + UNALIGNED_SIZES:
        batches, lone = {}, {}
        for fmt in FORMATS:
            srcs = [util.alloc_image(fmt, iw, ih, seed=1 + i) for i in range(2)]
            pairs = [(G.to_gpu(ctx, fmt, ow, oh, util.alloc_image(fmt, ow, oh)), G.to_gpu(ctx, fmt, iw, ih, srcs[i % 2])) for i in range(a.n)]
            batches[fmt] = sv.LanczosBatch(pairs)
            lone[fmt] = pairs[0]
            for _ in range(a.warmup):
                sv.usingContext(ctx, lambda c: batches[fmt].run(c))
        times = {fmt: [] for fmt in FORMATS}
        for _ in range(a.runs):                                  # the formats alternate: what disturbs one run disturbs its neighbours of every format
            for fmt in FORMATS:
                cv.check(lib.chv_event_record(ctx.handle, e0))
                batches[fmt].run(ctx)
                cv.check(lib.chv_event_record(ctx.handle, e1))
                cv.check(lib.chv_event_synchronize(e1))
                ms = C.c_float()
                cv.check(lib.chv_event_elapsed_ms(e0, e1, C.byref(ms)))
                times[fmt].append(ms.value * 1e3)
        walls = {}
        for fmt in FORMATS:
            gd, gs = lone[fmt]
            for _ in range(a.warmup):
                sv.usingContext(ctx, lambda c: sv.scaleLanczos(c, gd, gs))
            w = []
            for _ in range(a.runs):
                t = time.perf_counter()
                sv.usingContext(ctx, lambda c: sv.scaleLanczos(c, gd, gs))
                w.append((time.perf_counter() - t) * 1e6)
            walls[fmt] = statistics.median(w)
        base = statistics.median(times["bgra"])
        for fmt in FORMATS:
            med = statistics.median(times[fmt])
            nbytes = a.n * (payload_bytes(fmt, iw, ih) + payload_bytes(fmt, ow, oh))
            rate = nbytes / (med * 1e-6)
            results.append(dict(size=f"{iw}x{ih}->{ow}x{oh}", format=fmt, in_condition=(iw, ih, ow, oh) in SIZES, n=a.n, runs=a.runs, median_us=round(med, 1), min_us=round(min(times[fmt]), 1),
                                max_us=round(max(times[fmt]), 1), ratio_to_bgra=round(med / base, 3), algorithmic_gbs=round(rate / 1e9, 1),
                                share_of_peak=round(rate / PEAK, 4), lone_wall_us=round(walls[fmt], 1)))
        batches.clear(); lone.clear()
    print(f"{'size':>22} {'format':>6} {'median us':>10} {'min':>9} {'max':>9} {'ratio':>6} {'GB/s':>8} {'of 8 TB/s':>9} {'lone, wall us':>13}")
    for r in results:
        print(f"{r['size']:>22} {r['format']:>6} {r['median_us']:>10.1f} {r['min_us']:>9.1f} {r['max_us']:>9.1f} {r['ratio_to_bgra']:>6.3f} "
              f"{r['algorithmic_gbs']:>8.1f} {r['share_of_peak']:>9.4f} {r['lone_wall_us']:>13.1f}")
    ok = all(r["ratio_to_bgra"] <= 1.0 for r in results if r["in_condition"])
    for r in results:
        if not r["in_condition"] and r["format"] != "bgra":
            print(f"recorded, not in the condition: {r['size']} {r['format']} (rows that are not whole 16-byte vectors) ratio {r['ratio_to_bgra']:.3f}")
    print("condition: " + ("ok" if ok else "MISSED") + " (nv12 <= BGRA and y420p <= BGRA at both sizes)")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(dict(results=results, condition=ok), indent=1))
    sv.destroyComputeContext(ctx)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
