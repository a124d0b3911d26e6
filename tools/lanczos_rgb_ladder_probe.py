"""tools/lanczos_rgb_ladder_probe.py [--runs 7] [--window-ms 200] [--out file.json] — time of chv_scale_lanczos_rgb_ladder (every rendition of
every BGRA picture in one launch per route) and of the same renditions issued the way the library offered them before the entry existed: one
chv_scale_lanczos_batch call per rung for lists of two pictures or more, one chv_scale_lanczos call per rung for a lone picture.  Both sides
run in ONE process through one library, window by window in turn.  The bytes are the same — compared here, plane by plane, at the timed sizes —
so this is a time comparison only.

  1280x720  -> 640x360, 426x240, 320x180, 160x90        1 canvas and 16
  1920x1080 -> 1280x720, 854x480, 640x360, 320x180      1 picture and 16
  3840x2160 -> 1920x1080, 1280x720, 640x360             1 picture and 16

Every call of a window works on buffers of its own, rotated call by call, so that no call finds its source in the Infinity Cache because the
call before it read it.  A window holds nothing but C calls through ctypes with arguments made beforehand; it is timed twice over: by two
chv_event records around it (device time) and by the host's clock from the first call to the return of the wait for the second event (wall
time with a host wait).  After the windows every side is also timed call by call, each call followed by a host wait for it: `lone`, the
median wall time of 64 such calls, what a host sees that issues one rendition set and blocks on it.  A window's length is chosen per side so that it lasts about --window-ms; every side is warmed up first and the sides
alternate window by window.  A time is the median over --runs windows, in microseconds per rendition set (all rungs of all pictures count
once); `spread` is (max - min) / median of a side's windows.  There is no pass/fail ratio.  Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

CASES = [((1280, 720), [(640, 360), (426, 240), (320, 180), (160, 90)]),
         ((1920, 1080), [(1280, 720), (854, 480), (640, 360), (320, 180)]),
         ((3840, 2160), [(1920, 1080), (1280, 720), (640, 360)])]
COUNTS = [1, 16]
SETS = 32                   # pictures per source size: 32 lone ladders or two lists of 16 before a buffer comes round again


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import gpuutil as G
    import util
    from swiftvideo_amd import chipvideo as cv
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
        """(device us, wall us) per call of fn"""
        t0 = time.perf_counter()
        cv.check(lib.chv_event_record(handle, e0))
        for k in range(reps):
            fn(k)
        cv.check(lib.chv_event_record(handle, e1))
        cv.check(lib.chv_event_synchronize(e1))
        wall = time.perf_counter() - t0
        ms = C.c_float()
        cv.check(lib.chv_event_elapsed_ms(e0, e1, C.byref(ms)))
        return ms.value * 1e3 / reps, wall * 1e6 / reps

    def latency(fn, calls):
        """median wall us of ONE call followed by a host wait for it"""
        t = []
        for k in range(calls):
            t0 = time.perf_counter()
            fn(k)
            cv.check(lib.chv_event_record(handle, e1))
            cv.check(lib.chv_event_synchronize(e1))
            t.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(t)

    def images(samples):
        arr = (cv.Image * len(samples))()
        for i, s in enumerate(samples):
            arr[i] = sv._image_desc(s)
        return arr

    def at(arr, index):
        """a pointer to arr[index], as the signatures take a list"""
        return C.cast(C.addressof(arr) + index * C.sizeof(cv.Image), C.POINTER(cv.Image))

    results, keep = [], []
    for (iw, ih), rungs in CASES:
        geo, nr = f"{iw}x{ih}", len(rungs)
        host = util.alloc_image("bgra", iw, ih, seed=1)
        srcs = [G.to_gpu(ctx, "bgra", iw, ih, host) for _ in range(SETS)]
        s_img = images(srcs)
        # two sets of targets, one per side, so that the bytes can be compared afterwards
        fills = {side: [util.alloc_image("bgra", ow, oh, seed=2 + k) for (ow, oh) in rungs] for k, side in enumerate(("ladder", "calls"))}
        targets = {side: [[G.to_gpu(ctx, "bgra", ow, oh, fills[side][r]) for _ in range(SETS)] for r, (ow, oh) in enumerate(rungs)] for side in fills}
        t_img = {side: [images(t) for t in targets[side]] for side in targets}
        keep += [srcs, s_img, targets, t_img]
        sides = {}
        for n in COUNTS:
            groups = SETS // n
            lists = []
            for g in range(groups):
                arr = (cv.Image * (nr * n))()
                for r in range(nr):
                    for i in range(n):
                        arr[r * n + i] = t_img["ladder"][r][g * n + i]
                lists.append(arr)
            t_ptr = [[at(t_img["calls"][r], n * g) for g in range(groups)] for r in range(nr)]
            s_ptr = [at(s_img, n * g) for g in range(groups)]
            keep += [lists, t_ptr, s_ptr]

            def calls(k, n=n, groups=groups, t_ptr=t_ptr, s_ptr=s_ptr):
                g = k % groups
                for r in range(nr):
                    rc = lib.chv_scale_lanczos(handle, t_ptr[r][g], s_ptr[g]) if n == 1 else lib.chv_scale_lanczos_batch(handle, t_ptr[r][g], s_ptr[g], n)
                    if rc:
                        raise RuntimeError("a per-rung call failed")

            def ladder(k, n=n, groups=groups, lists=lists, s_ptr=s_ptr):
                g = k % groups
                if lib.chv_scale_lanczos_rgb_ladder(handle, lists[g], nr, s_ptr[g], n):
                    raise RuntimeError("the ladder failed")
            sides[(n, "ladder")] = ladder
            sides[(n, "calls")] = calls
        reps = {}
        for key, fn in sides.items():
            for _ in range(a.warmup):
                window(fn, 4)
            reps[key] = min(max(int(math.ceil(a.window_ms * 1e3 / max(window(fn, 8)[1], 1e-3))), 8), 20000)
        times = {key: [] for key in sides}
        lat = {key: [] for key in sides}
        for _ in range(a.runs):
            for key, fn in sides.items():
                times[key].append(window(fn, reps[key]))
        for _ in range(a.runs):
            for key, fn in sides.items():
                lat[key].append(latency(fn, 64))
        # the bytes, at the timed sizes: every group of both counts was written by both sides (reps >= 8 >= groups for n = 16; all 32 lone
        # pictures are written once more here)
        for k in range(SETS):
            sides[(1, "ladder")](k)
            sides[(1, "calls")](k)
        same = True
        for r, (ow, oh) in enumerate(rungs):
            for i in range(SETS):
                x, y = G.from_gpu(ctx, targets["ladder"][r][i], "bgra", ow, oh)[0], G.from_gpu(ctx, targets["calls"][r][i], "bgra", ow, oh)[0]
                same = same and bool(np.array_equal(x, y))
        for k in range(SETS // 16):
            sides[(16, "ladder")](k)
        for r, (ow, oh) in enumerate(rungs):
            for i in range(SETS):
                x, y = G.from_gpu(ctx, targets["ladder"][r][i], "bgra", ow, oh)[0], G.from_gpu(ctx, targets["calls"][r][i], "bgra", ow, oh)[0]
                same = same and bool(np.array_equal(x, y))
        for (n, side), t in times.items():
            dev, wall = [x[0] for x in t], [x[1] for x in t]
            md, mw = statistics.median(dev), statistics.median(wall)
            results.append(dict(source=geo, rungs=rungs, pictures=n, side=side, device_us=round(md, 2), device_spread=round((max(dev) - min(dev)) / md, 4),
                                wall_us=round(mw, 2), wall_spread=round((max(wall) - min(wall)) / mw, 4),
                                lone_call_us=round(statistics.median(lat[(n, side)]), 2),
                                lone_call_spread=round((max(lat[(n, side)]) - min(lat[(n, side)])) / statistics.median(lat[(n, side)]), 4), reps=reps[(n, side)], runs=a.runs, same_bytes=same))
        del srcs, targets
    print(f"# one process, one library, sides alternating; build flags: {cv.build_flags()}")
    print(f"{'source':>10} {'n':>3} {'side':>7} {'device us':>10} {'spread':>7} {'wall us':>10} {'spread':>7} {'lone us':>9} {'spread':>7} {'reps':>6} {'bytes':>6}")
    for r in results:
        print(f"{r['source']:>10} {r['pictures']:>3} {r['side']:>7} {r['device_us']:>10.2f} {r['device_spread']:>7.4f} {r['wall_us']:>10.2f} {r['wall_spread']:>7.4f} {r['lone_call_us']:>9.2f} {r['lone_call_spread']:>7.4f} "
              f"{r['reps']:>6} {'same' if r['same_bytes'] else 'DIFFER':>6}")
    print(f"{'source':>10} {'n':>3} {'ladder/calls device':>20} {'ladder/calls wall':>18} {'ladder/calls lone':>18}")
    for r in results:
        if r["side"] == "ladder":
            c = next(x for x in results if x["side"] == "calls" and x["source"] == r["source"] and x["pictures"] == r["pictures"])
            r["device_over_calls"], r["wall_over_calls"] = round(r["device_us"] / c["device_us"], 4), round(r["wall_us"] / c["wall_us"], 4)
            r["lone_over_calls"] = round(r["lone_call_us"] / c["lone_call_us"], 4)
            print(f"{r['source']:>10} {r['pictures']:>3} {r['device_over_calls']:>20.3f} {r['wall_over_calls']:>18.3f} {r['lone_over_calls']:>18.3f}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(dict(results=results), indent=1))
    sv.destroyComputeContext(ctx)
    return 0 if all(r["same_bytes"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
