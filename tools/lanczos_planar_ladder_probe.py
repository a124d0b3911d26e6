"""tools/lanczos_planar_ladder_probe.py [--runs 15] [--window-ms 5] [--out file.json] — device time of chv_scale_lanczos_ladder (the 4:2:0
ladder: nv12 -> nv12, y420p -> y420p) against what a host did for the same ladder before it existed, in ONE process on one device.  Cases:

  1080p3   1920x1080 -> {1280x720, 854x480, 640x360}             all on the wave-per-strip route
  1080p4   the same plus 426x240                                  (28 taps: the tile route, a second launch)
  2160p3   3840x2160 -> {1920x1080, 1280x720, 854x480}            the last rung takes the tile route

each for nv12 and y420p, for one picture and for 16.  Sides of a case:

  ladder   chv_scale_lanczos_ladder: every rung of every picture in one call
  calls    one call per rung: chv_scale_lanczos for one picture, chv_scale_lanczos_batch for 16
  calls2   the same calls again, as a side of its own: what two runs of identical code differ by inside this process is the spread the
           condition allows

Every side builds its descriptors ONCE, outside the windows: a window holds nothing but C calls through ctypes with arguments made beforehand
(a window is back-to-back enqueues, so a host-bound side measures host time — Python that builds descriptors must not be part of one side).

A time is the median over `runs` windows; a window is `reps` back-to-back ladders between two chv_event records, `reps` chosen per side so that
the window lasts about --window-ms (well past the launch overhead); every side is warmed up first, and the sides alternate window by window, so
what disturbs one window disturbs its neighbours of every side.  Prints a table with the launches each side made (the ladder's from the
"lanczos_planar_ladder_launches" counter), and per case "ok" when ladder <= mean(calls, calls2) x (1 + spread), spread = |calls - calls2| /
min(calls, calls2): a caller must never be slower through the ladder than without it.  --diagnose adds cases that take the 2160p ladder apart
(nv12 only; reported like the others, not part of the condition): its two strip rungs alone (tap classes 12 and 22: planar_lanczos_ladder<22>,
four waves), the class-12 rung alone (<12>, five waves, as its single call) and its tile rung alone.
Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import gpuutil as G          # noqa: E402
import util                  # noqa: E402
from swiftvideo_amd import chipvideo as cv       # noqa: E402
from swiftvideo_amd import compute as sv         # noqa: E402

CASES = [("1080p3", (1920, 1080), [(1280, 720), (854, 480), (640, 360)]),
         ("1080p4", (1920, 1080), [(1280, 720), (854, 480), (640, 360), (426, 240)]),
         ("2160p3", (3840, 2160), [(1920, 1080), (1280, 720), (854, 480)])]
DIAGNOSE = [("d2160s2", (3840, 2160), [(1920, 1080), (1280, 720)]),       # the strip launch of 2160p3: classes 12 + 22, <22> at four waves
            ("d2160s1", (3840, 2160), [(1920, 1080)]),                    # class 12 alone: <12> at five waves, as the single call
            ("d2160t1", (3840, 2160), [(854, 480)])]                      # the tile launch of 2160p3
FORMATS = ["nv12", "y420p"]
SIDES = ["ladder", "calls", "calls2"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window-ms", type=float, default=5.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--cases", default=None, help="comma-separated case names (default: all)")
    ap.add_argument("--diagnose", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = cv.load()
    ctx = sv.makeComputeContext(forType="GPU")

    def event():
        h = C.c_void_p()
        cv.check(lib.chv_event_create(ctx.handle, C.byref(h)))
        return h
    e0, e1 = event(), event()

    def window(fn, reps):
        """microseconds per ladder over one window of `reps` ladders"""
        cv.check(lib.chv_event_record(ctx.handle, e0))
        for _ in range(reps):
            fn()
        cv.check(lib.chv_event_record(ctx.handle, e1))
        cv.check(lib.chv_event_synchronize(e1))
        ms = C.c_float()
        cv.check(lib.chv_event_elapsed_ms(e0, e1, C.byref(ms)))
        return ms.value * 1e3 / reps

    results = []
    have_src = {}
    handle = ctx.handle
    for name, (iw, ih), sizes in sorted(CASES + (DIAGNOSE if a.diagnose else []), key=lambda c: -c[1][0]):      # (one source size after the other)
        if a.cases and name not in a.cases.split(","):
            continue
        gated = not name.startswith("d")
        for fmt in (FORMATS if gated else FORMATS[:1]):
            if (fmt, iw, ih) not in have_src:
                have_src.clear()                                   # (one source size and format at a time)
                one = util.alloc_image(fmt, iw, ih, seed=1)
                have_src[(fmt, iw, ih)] = [G.to_gpu(ctx, fmt, iw, ih, [np_roll(p, i) for p in one]) for i in range(a.batch)]
            srcs = have_src[(fmt, iw, ih)]
            rungs = [[G.to_gpu(ctx, fmt, w, h, util.alloc_image(fmt, w, h)) for _ in range(a.batch)] for w, h in sizes]
            for n in (1, a.batch):
                # every side's descriptors, once: the windows below make nothing but C calls
                ladder = sv.LanczosLadder([r[:n] for r in rungs], srcs[:n])
                ladder_fn, ld, ls, lr = lib.chv_scale_lanczos_ladder, ladder._d, ladder._s, ladder.n_rungs

                def run_ladder():
                    if ladder_fn(handle, ld, lr, ls, n):
                        raise RuntimeError("chv_scale_lanczos_ladder failed")
                if n == 1:
                    descs = [(sv._image_desc(r[0]), sv._image_desc(srcs[0])) for r in rungs]
                    args = [(C.byref(d), C.byref(s)) for d, s in descs]
                    single = lib.chv_scale_lanczos

                    def calls():
                        for d, s in args:
                            if single(handle, d, s):
                                raise RuntimeError("chv_scale_lanczos failed")
                else:
                    batches = [sv.LanczosBatch(list(zip(r[:n], srcs[:n]))) for r in rungs]
                    bargs = [(b._d, b._s) for b in batches]
                    batch = lib.chv_scale_lanczos_batch

                    def calls():
                        for d, s in bargs:
                            if batch(handle, d, s, n):
                                raise RuntimeError("chv_scale_lanczos_batch failed")
                launches_calls = len(sizes)
                sides = {"ladder": run_ladder, "calls": calls, "calls2": calls}
                before = cv.get_counter("lanczos_planar_ladder_launches")
                run_ladder()
                launches_ladder = cv.get_counter("lanczos_planar_ladder_launches") - before
                reps = {}
                for s in SIDES:                                    # warm-up of every side, and the length of its window
                    for _ in range(a.warmup):
                        window(sides[s], 3)
                    reps[s] = min(max(int(math.ceil(a.window_ms * 1e3 / max(window(sides[s], 10), 1e-3))), 10), 2000)
                times = {s: [] for s in SIDES}
                for _ in range(a.runs):
                    for s in SIDES:
                        times[s].append(window(sides[s], reps[s]))
                med = {s: statistics.median(times[s]) for s in SIDES}
                spread = abs(med["calls"] - med["calls2"]) / min(med["calls"], med["calls2"])
                calls_med = 0.5 * (med["calls"] + med["calls2"])
                ok = med["ladder"] <= calls_med * (1.0 + spread)
                results.append(dict(case=name, source=f"{iw}x{ih}", rungs=[f"{w}x{h}" for w, h in sizes], target=fmt, n=n, runs=a.runs, reps=reps,
                                    us={s: round(med[s], 2) for s in SIDES},
                                    window_spread={s: round((max(times[s]) - min(times[s])) / med[s], 4) for s in SIDES},
                                    same_code_spread=round(spread, 4), ladder_over_calls=round(med["ladder"] / calls_med, 4),
                                    launches=dict(ladder=int(launches_ladder), calls=launches_calls), ok=bool(ok), gated=gated))
    print(f"{'case':>8} {'fmt':>6} {'n':>3} {'ladder us':>10} {'calls us':>9} {'calls2 us':>9} {'ladder/calls':>12} {'spread':>7} {'launches':>9}")
    for r in results:
        u = r["us"]
        print(f"{r['case']:>8} {r['target']:>6} {r['n']:>3} {u['ladder']:>10.2f} {u['calls']:>9.2f} {u['calls2']:>9.2f} {r['ladder_over_calls']:>12.3f} "
              f"{r['same_code_spread']:>7.4f} {r['launches']['ladder']:>4} /{r['launches']['calls']:>3}  {'ok' if r['ok'] else 'MISSED'}")
    ok = all(r["ok"] for r in results if r["gated"])
    print("condition: " + ("ok" if ok else "MISSED") + " (ladder <= the calls within the spread of two runs of the calls, every case)")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(dict(results=results, condition=ok), indent=1))
    sv.destroyComputeContext(ctx)
    return 0 if ok else 1


def np_roll(plane, i):
    """picture i of a case: the seeded plane rolled by i rows (sixteen 2160p planes are not drawn sixteen times)"""
    import numpy as np
    return np.ascontiguousarray(np.roll(plane, i, axis=0))


if __name__ == "__main__":
    sys.exit(main())
