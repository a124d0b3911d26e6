"""tools/lanczos_from_yuv_ladder_probe.py [--yardstick] [--against yardstick.json] [--runs 7] [--window-ms 300] [--out file.json] — device time
of chv_scale_lanczos_from_yuv_ladder (every BGRA rendition of every NV12 or y420p picture in one launch per route) and of the same renditions
issued the way the PARENT commit offers: one chv_scale_lanczos_from_yuv_batch call per rung.  The bytes are the same; a time comparison.

  geometries  1920x1080 and 3840x2160 -> 1280x720, 960x540, 640x360 and 320x180; both packings; 1 picture and 16

A process measures one library.  Without --yardstick it is the tree's own: side `ladder`, and as context side `calls` (the per-rung batch
calls through the tree's library).  With --yardstick the library is the one CHV_LIB names — the parent's, which does not have the new entry:
the binding is loaded without it and the per-rung calls are measured TWICE, as sides `calls` and `calls_again` of the same run (an A/A pair:
the same-code spread, what the probe itself cannot tell apart).  Never the new code as its own yardstick.  --against reads a yardstick's
--out file and prints the ladder's time over the calls' beside that spread; a row where the ladder is slower than the calls beyond the
spread is marked SLOWER (callers keep the calls there).  The margin is the measured spread: nothing tighter or looser is fixed in advance.

Every call of a window works on buffers of its own, rotated call by call, so that no call finds its source in the Infinity Cache because the
call before it read it.  A window holds nothing but C calls through ctypes with arguments made beforehand, between two chv_event records; its
length is chosen per side so that it lasts about --window-ms; every side is warmed up first and the sides alternate window by window.  A time
is the median over --runs windows, in microseconds per rendition set (the four rungs of all pictures count once); `spread` is (max - min) /
median of a side's windows.  Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

SOURCES = [(1920, 1080), (3840, 2160)]
RUNGS = [(1280, 720), (960, 540), (640, 360), (320, 180)]
FORMATS = ["nv12", "y420p"]
COUNTS = [1, 16]
SETS = 32                   # pictures per (source size, format): 32 lone ladders or two lists of 16 before a buffer comes round again
NEW = ("chv_scale_lanczos_from_yuv_ladder",)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--against", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=300.0)
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

    def images(samples):
        arr = (cv.Image * len(samples))()
        for i, s in enumerate(samples):
            arr[i] = sv._image_desc(s)
        return arr

    def at(arr, index):
        """a pointer to arr[index], as the signatures take a list"""
        return C.cast(C.addressof(arr) + index * C.sizeof(cv.Image), C.POINTER(cv.Image))

    opts = cv.KernelOpts(colorspace=cv.CSC_BT601_LIMITED)
    nr = len(RUNGS)
    targets = [[G.to_gpu(ctx, "bgra", ow, oh, util.alloc_image("bgra", ow, oh)) for _ in range(SETS)] for (ow, oh) in RUNGS]
    t_img = [images(t) for t in targets]                    # per rung: the targets of picture 0 .. SETS - 1
    keep = [targets, t_img, opts]
    # ladder lists, dsts[r * n + i]: for n = 1 one per picture, for n = 16 one per group of 16
    lists = {}
    for n in COUNTS:
        per = []
        for g in range(SETS // n):
            arr = (cv.Image * (nr * n))()
            for r in range(nr):
                for i in range(n):
                    arr[r * n + i] = t_img[r][g * n + i]
            per.append(arr)
        lists[n] = per
    t_ptr = {n: [[at(t_img[r], n * g) for g in range(SETS // n)] for r in range(nr)] for n in COUNTS}
    keep += [lists, t_ptr]
    sides = {}
    for (iw, ih) in SOURCES:
        geo = f"{iw}x{ih}"
        for fmt in FORMATS:
            host = util.alloc_image(fmt, iw, ih, seed=1)
            srcs = [G.to_gpu(ctx, fmt, iw, ih, host) for _ in range(SETS)]
            s_img = images(srcs)
            keep += [srcs, s_img]
            s_ptr = {n: [at(s_img, n * g) for g in range(SETS // n)] for n in COUNTS}
            keep.append(s_ptr)
            for n in COUNTS:
                groups = SETS // n

                def calls(k, n=n, groups=groups, s_ptr=s_ptr):
                    g = k % groups
                    for r in range(nr):
                        if lib.chv_scale_lanczos_from_yuv_batch(handle, t_ptr[n][r][g], s_ptr[n][g], n, C.byref(opts)):
                            raise RuntimeError("a per-rung call failed")

                def ladder(k, n=n, groups=groups, s_ptr=s_ptr):
                    g = k % groups
                    if lib.chv_scale_lanczos_from_yuv_ladder(handle, lists[n][g], nr, s_ptr[n][g], n, C.byref(opts)):
                        raise RuntimeError("the ladder failed")
                if a.yardstick:
                    sides[(geo, fmt, n, "calls")] = calls
                    sides[(geo, fmt, n, "calls_again")] = calls
                else:
                    sides[(geo, fmt, n, "ladder")] = ladder
                    sides[(geo, fmt, n, "calls")] = calls

    reps = {}
    for key, fn in sides.items():
        for _ in range(a.warmup):
            window(fn, 4)
        reps[key] = min(max(int(math.ceil(a.window_ms * 1e3 / max(window(fn, 8), 1e-3))), 8), 20000)
    times = {key: [] for key in sides}
    for _ in range(a.runs):
        for key, fn in sides.items():
            times[key].append(window(fn, reps[key]))
    results = []
    for (geo, fmt, n, side), t in times.items():
        med = statistics.median(t)
        results.append(dict(source=geo, format=fmt, pictures=n, side=side, us=round(med, 2), spread=round((max(t) - min(t)) / med, 4),
                            reps=reps[(geo, fmt, n, side)], runs=a.runs))
    what = "yardstick (the library CHV_LIB names: one chv_scale_lanczos_from_yuv_batch call per rung, measured twice)" if a.yardstick else "the tree's library"
    print(f"# {what}; rungs {RUNGS}; build flags: {cv.build_flags()}")
    print(f"{'source':>10} {'format':>6} {'n':>3} {'side':>12} {'us':>10} {'spread':>7} {'reps':>6}")
    for r in results:
        print(f"{r['source']:>10} {r['format']:>6} {r['pictures']:>3} {r['side']:>12} {r['us']:>10.2f} {r['spread']:>7.4f} {r['reps']:>6}")
    if a.against:
        base = {(r["source"], r["format"], r["pictures"], r["side"]): r["us"] for r in json.loads(Path(a.against).read_text())["results"]}
        print(f"{'source':>10} {'format':>6} {'n':>3} {'ladder us':>10} {'calls us':>10} {'ratio':>7} {'A/A':>7} {'own calls us':>13}")
        for r in results:
            if r["side"] != "ladder":
                continue
            key = (r["source"], r["format"], r["pictures"])
            ch, again = base[key + ("calls",)], base[key + ("calls_again",)]
            aa = abs(ch - again) / min(ch, again)
            own = next(x["us"] for x in results if x["side"] == "calls" and (x["source"], x["format"], x["pictures"]) == key)
            r["calls_us"], r["calls_again_us"], r["over_calls"], r["calls_aa"] = ch, again, round(r["us"] / ch, 4), round(aa, 4)
            r["slower"] = bool(r["us"] > max(ch, again) * (1 + aa))
            print(f"{r['source']:>10} {r['format']:>6} {r['pictures']:>3} {r['us']:>10.2f} {ch:>10.2f} {r['over_calls']:>7.3f} {aa:>7.4f} {own:>13.2f}"
                  f"{'  SLOWER' if r['slower'] else ''}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(dict(yardstick=a.yardstick, rungs=RUNGS, results=results), indent=1))
    sv.destroyComputeContext(ctx)
    return 0


if __name__ == "__main__":
    sys.exit(main())
