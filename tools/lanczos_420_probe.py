"""tools/lanczos_420_probe.py [--yardstick] [--against yardstick.json] [--runs 9] [--window-ms 20] [--out file.json] — device time of the 4:2:0
conversion entries (chv_scale_lanczos_420, chv_scale_lanczos_420_ladder) for all four (source packing, target packing) pairs, and of the
yardstick they are held against: the same-format calls of the same geometry through the PARENT commit's library in the same session.

  lone      1920x1080 -> 1280x720, one call, one picture
  ladder1   1920x1080 -> {1280x720, 854x480, 640x360}, one picture
  ladder16  the same for 16 pictures

A process measures one library.  Without --yardstick it is the tree's own, through the new entries (same-format pairs are forwarded by them).
With --yardstick the library is the one CHV_LIB names — the parent's, which does not have the new entries: the binding is loaded without them and
only nv12 -> nv12 and y420p -> y420p are measured, through chv_scale_lanczos and chv_scale_lanczos_ladder.  Never the new code as its own yardstick.
--against reads a yardstick's --out file and prints, per cross pair, its time over the slower same-format pair's (expected about 1: the same
arithmetic per output byte) and THE GATE: a cross ladder slower than the two same-format ladders of its geometry added together is a defect
(exit status 1).

Every call of a window works on buffers of its own: 64 sources and 64 sets of targets per format, some 700 MB, rotated call by call, so that no
call finds its source in the 256 MB Infinity Cache because the call before it read it.  A window holds nothing but C calls through ctypes with
arguments made beforehand, between two chv_event records; its length is chosen per side so that it lasts about --window-ms; every side is
warmed up first and the sides alternate window by window.  A time is the median over --runs windows, in microseconds per call; `spread` is
(max - min) / median of a side's windows.  Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

SRC = (1920, 1080)
RUNGS = [(1280, 720), (854, 480), (640, 360)]
FORMATS = ["nv12", "y420p"]
CASES = ["lone", "ladder1", "ladder16"]
SETS = 64
NEW = ("chv_scale_lanczos_420", "chv_scale_lanczos_420_ladder")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--against", default=None)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from swiftvideo_amd import chipvideo as cv
    if a.yardstick:
        for name in NEW:
            cv._SIGNATURES.pop(name)
    import gpuutil as G
    import util
    from swiftvideo_amd import compute as sv
    lib = cv.load()
    ctx = sv.makeComputeContext(forType="GPU")
    handle = ctx.handle

    def event():
        h = C.c_void_p()
        cv.check(lib.chv_event_create(handle, C.byref(h)))
        return h
    e0, e1 = event(), event()

    def window(fn, reps):
        cv.check(lib.chv_event_record(handle, e0))
        for k in range(reps):
            fn(k)
        cv.check(lib.chv_event_record(handle, e1))
        cv.check(lib.chv_event_synchronize(e1))
        ms = C.c_float()
        cv.check(lib.chv_event_elapsed_ms(e0, e1, C.byref(ms)))
        return ms.value * 1e3 / reps

    srcs, dsts = {}, {}
    for fmt in FORMATS:
        host = util.alloc_image(fmt, *SRC, seed=1)
        srcs[fmt] = [G.to_gpu(ctx, fmt, *SRC, host) for _ in range(SETS)]
        dsts[fmt] = [[G.to_gpu(ctx, fmt, w, h, util.alloc_image(fmt, w, h)) for _ in range(SETS)] for w, h in RUNGS]

    sides, keep = {}, []
    for sfmt in FORMATS:
        for dfmt in FORMATS:
            if a.yardstick and sfmt != dfmt:
                continue
            single = lib.chv_scale_lanczos if a.yardstick else lib.chv_scale_lanczos_420
            ladder = lib.chv_scale_lanczos_ladder if a.yardstick else lib.chv_scale_lanczos_420_ladder
            lone = [(sv._image_desc(dsts[dfmt][0][k]), sv._image_desc(srcs[sfmt][k])) for k in range(SETS)]
            lone_args = [(C.byref(d), C.byref(s)) for d, s in lone]
            one = [sv.LanczosLadder([[r[k]] for r in dsts[dfmt]], [srcs[sfmt][k]]) for k in range(SETS)]
            many = [sv.LanczosLadder([r[16 * j: 16 * j + 16] for r in dsts[dfmt]], srcs[sfmt][16 * j: 16 * j + 16]) for j in range(SETS // 16)]
            keep += [lone, one, many]

            def run_lone(k, single=single, args=lone_args):
                d, s = args[k % SETS]
                if single(handle, d, s):
                    raise RuntimeError("the single call failed")

            def run_one(k, ladder=ladder, ls=one):
                l = ls[k % SETS]
                if ladder(handle, l._d, 3, l._s, 1):
                    raise RuntimeError("the ladder of one picture failed")

            def run_many(k, ladder=ladder, ls=many):
                l = ls[k % len(ls)]
                if ladder(handle, l._d, 3, l._s, 16):
                    raise RuntimeError("the ladder of 16 pictures failed")
            for case, fn in zip(CASES, (run_lone, run_one, run_many)):
                sides[(f"{sfmt}->{dfmt}", case)] = fn

    reps = {}
    for key, fn in sides.items():
        for _ in range(a.warmup):
            window(fn, 4)
        reps[key] = min(max(int(math.ceil(a.window_ms * 1e3 / max(window(fn, 8), 1e-3))), 8), 4000)
    times = {key: [] for key in sides}
    for _ in range(a.runs):
        for key, fn in sides.items():
            times[key].append(window(fn, reps[key]))
    results = []
    for (pair, case), t in times.items():
        med = statistics.median(t)
        results.append(dict(pair=pair, case=case, us=round(med, 2), spread=round((max(t) - min(t)) / med, 4), reps=reps[(pair, case)], runs=a.runs))
    what = "yardstick (the library CHV_LIB names, same-format calls)" if a.yardstick else "the tree's library, the 4:2:0 conversion entries"
    print(f"# {what}; build flags: {cv.build_flags()}")
    print(f"{'pair':>14} {'case':>9} {'us':>10} {'spread':>7} {'reps':>5}")
    for r in results:
        print(f"{r['pair']:>14} {r['case']:>9} {r['us']:>10.2f} {r['spread']:>7.4f} {r['reps']:>5}")
    ok = True
    if a.against:
        base = {(r["pair"], r["case"]): r["us"] for r in json.loads(Path(a.against).read_text())["results"]}
        mine = {(r["pair"], r["case"]): r["us"] for r in results}
        print(f"{'pair':>14} {'case':>9} {'us':>10} {'/ slower same-format':>21} {'/ sum of both':>14}")
        for r in results:
            s, d = r["pair"].split("->")
            both = [base[(f"{f}->{f}", r["case"])] for f in FORMATS]
            r["over_slower_same_format"], r["over_sum"] = round(r["us"] / max(both), 4), round(r["us"] / sum(both), 4)
            if s == d:
                r["over_parent"] = round(r["us"] / base[(r["pair"], r["case"])], 4)
            gate = s != d and r["case"] != "lone" and r["us"] > sum(both)
            ok = ok and not gate
            print(f"{r['pair']:>14} {r['case']:>9} {r['us']:>10.2f} {r['over_slower_same_format']:>21.3f} {r['over_sum']:>14.3f}{'  DEFECT' if gate else ''}")
        assert mine
        print("gate: " + ("ok" if ok else "MISSED") + " (no cross ladder slower than the two same-format ladders of its geometry added together)")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(dict(yardstick=a.yardstick, results=results, gate=ok), indent=1))
    sv.destroyComputeContext(ctx)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
