"""tools/lanczos_to_yuv_probe.py [--runs 15] [--window-ms 5] [--out file.json] — device time of chv_scale_lanczos_to_yuv against what a host
had for the same job before it existed, at 3840x2160 -> 1920x1080, 1920x1080 -> 1280x720 and 1366x768 -> 854x480, single and as a batch of 16,
into nv12 and y420p, in ONE process on one device.  Sides of a case:

  new     chv_scale_lanczos_to_yuv (single) / chv_scale_lanczos_to_yuv_batch (16)
  chain   the two launches of before: chv_scale_lanczos into a BGRA temporary of the target size + a full-canvas img_bgra_{nv12,y420p}_int tick
          (chv_composite; 16: chv_scale_lanczos_batch + one batch of 16 ticks).  Its bytes are not `new`'s (the tick samples the temporary
          bilinearly at gid - 0.5): a cost comparison only.
  chain2  the same chain again, as a side of its own: what two runs of identical code differ by inside this call is the spread (a)'s condition allows
  bgra    chv_scale_lanczos BGRA -> BGRA of the same geometry (reported, not gated)

A time is the median over `runs` windows; a window is `reps` back-to-back calls between two chv_event records, `reps` chosen per side so that the
window lasts about --window-ms (well past the launch overhead); every side is warmed up first, and the sides alternate window by window, so what
disturbs one window disturbs its neighbours of every side.  Prints a table, and per case "(a) ok" when new <= chain x (1 + spread), spread =
|chain - chain2| / min(chain, chain2).  Needs a GPU: there is no fall-back."""
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

SIZES = [(3840, 2160, 1920, 1080), (1920, 1080, 1280, 720), (1366, 768, 854, 480)]
TARGETS = ["nv12", "y420p"]
SIDES = ["new", "chain", "bgra", "chain2"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window-ms", type=float, default=5.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
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
        """microseconds per call over one window of `reps` calls"""
        cv.check(lib.chv_event_record(ctx.handle, e0))
        for _ in range(reps):
            fn()
        cv.check(lib.chv_event_record(ctx.handle, e1))
        cv.check(lib.chv_event_synchronize(e1))
        ms = C.c_float()
        cv.check(lib.chv_event_elapsed_ms(e0, e1, C.byref(ms)))
        return ms.value * 1e3 / reps

    results = []
    for iw, ih, ow, oh in SIZES:
        srcs = [G.to_gpu(ctx, "bgra", iw, ih, util.alloc_image("bgra", iw, ih, seed=1 + i)) for i in range(a.batch)]
        temps = [G.to_gpu(ctx, "bgra", ow, oh, util.alloc_image("bgra", ow, oh)) for _ in range(a.batch)]
        outs = [G.to_gpu(ctx, "bgra", ow, oh, util.alloc_image("bgra", ow, oh)) for _ in range(a.batch)]
        ue = util.full_canvas_uniforms((ow, oh), (ow, oh))
        for fmt in TARGETS:
            k_int = sv.defaultComputeKernelFromString(f"img_bgra_{fmt}_int")
            dsts = [G.to_gpu(ctx, fmt, ow, oh, util.alloc_image(fmt, ow, oh)) for _ in range(a.batch)]
            for n in (1, a.batch):
                if n == 1:
                    def chain():
                        sv.scaleLanczos(ctx, temps[0], srcs[0])
                        sv.compositeTick(ctx, dsts[0], [(k_int, temps[0], ue, 0)], True)
                    sides = {"new": lambda: sv.scaleLanczosToYuv(ctx, dsts[0], srcs[0]), "chain": chain, "chain2": chain,
                             "bgra": lambda: sv.scaleLanczos(ctx, outs[0], srcs[0])}
                    keep = None
                else:
                    new_b = sv.LanczosToYuvBatch(list(zip(dsts[:n], srcs[:n])))
                    tmp_b = sv.LanczosBatch(list(zip(temps[:n], srcs[:n])))
                    out_b = sv.LanczosBatch(list(zip(outs[:n], srcs[:n])))
                    tick_b = sv.TickBatch(ctx, [(dsts[i], True, [(k_int, temps[i], ue, 0)]) for i in range(n)])
                    keep = (new_b, tmp_b, out_b, tick_b)

                    def chain():
                        tmp_b.run(ctx)
                        tick_b.run(ctx)
                    sides = {"new": lambda: new_b.run(ctx), "chain": chain, "chain2": chain, "bgra": lambda: out_b.run(ctx)}
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
                spread = abs(med["chain"] - med["chain2"]) / min(med["chain"], med["chain2"])
                chain_med = 0.5 * (med["chain"] + med["chain2"])
                ok = med["new"] <= chain_med * (1.0 + spread)
                results.append(dict(size=f"{iw}x{ih}->{ow}x{oh}", target=fmt, n=n, runs=a.runs, reps=reps,
                                    us={s: round(med[s], 2) for s in SIDES},
                                    window_spread={s: round((max(times[s]) - min(times[s])) / med[s], 4) for s in SIDES},
                                    same_code_spread=round(spread, 4), new_over_chain=round(med["new"] / chain_med, 4),
                                    new_over_bgra=round(med["new"] / med["bgra"], 4), a_ok=bool(ok)))
                if keep is not None:                               # (every window ended in a wait: nothing of the batch is in flight)
                    keep[3].destroy()
    print(f"{'size':>22} {'to':>6} {'n':>3} {'new us':>9} {'chain us':>9} {'chain2 us':>9} {'bgra us':>9} {'new/chain':>9} {'new/bgra':>9} {'spread':>7}  (a)")
    for r in results:
        u = r["us"]
        print(f"{r['size']:>22} {r['target']:>6} {r['n']:>3} {u['new']:>9.2f} {u['chain']:>9.2f} {u['chain2']:>9.2f} {u['bgra']:>9.2f} "
              f"{r['new_over_chain']:>9.3f} {r['new_over_bgra']:>9.3f} {r['same_code_spread']:>7.4f}  {'ok' if r['a_ok'] else 'MISSED'}")
    ok = all(r["a_ok"] for r in results)
    print("condition (a): " + ("ok" if ok else "MISSED") + " (new <= chain within the spread of two runs of the chain, every case)")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(dict(results=results, condition_a=ok), indent=1))
    sv.destroyComputeContext(ctx)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
