"""tools/lanczos_hbd_probe.py [--runs 5] [--window-ms 100] [--sets 16] [--out file.json] — device time of chv_scale_lanczos_hbd_to_420 /
chv_scale_lanczos_hbd_to_420_ladder for the two 10-bit sources (p010, y420p10) into both targets (nv12, y420p), beside the yardstick:
chv_scale_lanczos_420 / _420_ladder, y420p -> nv12, for the same picture and target sizes in the same process — the same taps on half the
source bytes.  There is no earlier GPU path for these formats: no regression bar, no threshold; the probe reports.

  geometries  1920x1080 -> 1280x720 and 1920x1080 -> 1920x1080
  cases       one    one call, one picture            (both geometries)
              rungs  1920x1080 -> {1280x720, 854x480, 640x360, 426x240}: one ladder call of one picture (`one`) and of 16 pictures (`n16`)

Every call of a window works on buffers of its own (--sets of them, rotated call by call).  A window holds nothing but C calls through ctypes
with arguments made beforehand, between two chv_event records; its length is chosen per side so that it lasts about --window-ms; every side is
warmed up first and the sides ALTERNATE window by window.  A time is the median over --runs windows, in microseconds per call; `spread` is
(max - min) / median of a side's windows.  Per cell the probe prints its time over the yardstick's and its BYTE ratio — (source + target bytes)
over the yardstick's.  Needs a GPU: there is no fall-back."""
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
GEOMETRIES = {"720p": [(1280, 720)], "1080p": [(1920, 1080)], "rungs": [(1280, 720), (854, 480), (640, 360), (426, 240)]}
TARGETS = ["nv12", "y420p"]
YARD = ("y420p", "nv12")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gpuutil as G
    import hbd_formats as H
    import util
    from swiftvideo_amd import chipvideo as cv
    from swiftvideo_amd import compute as sv
    lib = cv.load()
    ctx = sv.makeComputeContext(forType="GPU")
    handle = ctx.handle
    sets = a.sets
    assert sets >= 16 and sets % 16 == 0

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

    srcs = {"y420p": [G.to_gpu(ctx, "y420p", *SRC, util.alloc_image("y420p", *SRC, seed=1)) for _ in range(sets)]}
    codes = H.random_codes(*SRC, 1)
    for fmt in H.FORMATS:
        host = H.pack(fmt, *codes, seed=1)
        srcs[fmt] = [H.to_gpu(ctx, fmt, *SRC, host) for _ in range(sets)]
    sizes = sorted({s for g in GEOMETRIES.values() for s in g})
    dsts = {(fmt, s): [G.to_gpu(ctx, fmt, *s, util.alloc_image(fmt, *s)) for _ in range(sets)] for fmt in TARGETS for s in sizes}

    sides, keep = {}, []
    for sfmt, dfmt in [YARD] + [(s, d) for s in H.FORMATS for d in TARGETS]:
        yard = (sfmt, dfmt) == YARD
        single = lib.chv_scale_lanczos_420 if yard else lib.chv_scale_lanczos_hbd_to_420
        ladder = lib.chv_scale_lanczos_420_ladder if yard else lib.chv_scale_lanczos_hbd_to_420_ladder
        for geo, rungs in GEOMETRIES.items():
            if geo != "rungs":
                descs = [(sv._image_desc(dsts[(dfmt, rungs[0])][k]), sv._image_desc(srcs[sfmt][k])) for k in range(sets)]
                args = [(C.byref(d), C.byref(s)) for d, s in descs]
                keep.append(descs)

                def run_one(k, single=single, args=args):
                    d, s = args[k % len(args)]
                    if single(handle, d, s):
                        raise RuntimeError("the single call failed")
                sides[(f"{sfmt}->{dfmt}", geo, "one")] = run_one
            else:
                ones = [sv.LanczosLadder([[dsts[(dfmt, s)][k]] for s in rungs], [srcs[sfmt][k]]) for k in range(sets)]
                many = [sv.LanczosLadder([dsts[(dfmt, s)][16 * j: 16 * j + 16] for s in rungs], srcs[sfmt][16 * j: 16 * j + 16]) for j in range(sets // 16)]
                keep += [ones, many]

                def run_rungs(k, ladder=ladder, ls=ones, n=len(rungs)):
                    l = ls[k % len(ls)]
                    if ladder(handle, l._d, n, l._s, 1):
                        raise RuntimeError("the ladder failed")

                def run_rungs16(k, ladder=ladder, ls=many, n=len(rungs)):
                    l = ls[k % len(ls)]
                    if ladder(handle, l._d, n, l._s, 16):
                        raise RuntimeError("the ladder of 16 pictures failed")
                sides[(f"{sfmt}->{dfmt}", geo, "one")] = run_rungs
                sides[(f"{sfmt}->{dfmt}", geo, "n16")] = run_rungs16

    reps = {}
    for key, fn in sides.items():
        for _ in range(a.warmup):
            window(fn, 4)
        reps[key] = min(max(int(math.ceil(a.window_ms * 1e3 / max(window(fn, 8), 1e-3))), 8), 20000)
    times = {key: [] for key in sides}
    for _ in range(a.runs):                     # the sides alternate window by window
        for key, fn in sides.items():
            times[key].append(window(fn, reps[key]))
    med = {key: statistics.median(t) for key, t in times.items()}
    results = []
    print(f"# build flags: {cv.build_flags()}")
    print(f"{'pair':>15} {'geometry':>8} {'case':>5} {'us':>10} {'spread':>7} {'reps':>6} {'/ yardstick':>12} {'byte ratio':>11}")
    for (pair, geo, case), t in times.items():
        sfmt, dfmt = pair.split("->")
        yard = med[(f"{YARD[0]}->{YARD[1]}", geo, case)]
        out_bytes = sum(1.5 * w * h for w, h in GEOMETRIES[geo])
        src_bytes = (1.5 if sfmt == "y420p" else 3.0) * SRC[0] * SRC[1]
        ratio = (src_bytes + out_bytes) / (1.5 * SRC[0] * SRC[1] + out_bytes)
        r = dict(pair=pair, geometry=geo, case=case, us=round(med[(pair, geo, case)], 2), spread=round((max(t) - min(t)) / med[(pair, geo, case)], 4),
                 reps=reps[(pair, geo, case)], runs=a.runs, over_yardstick=round(med[(pair, geo, case)] / yard, 4), byte_ratio=round(ratio, 4))
        results.append(r)
        print(f"{pair:>15} {geo:>8} {case:>5} {r['us']:>10.2f} {r['spread']:>7.4f} {r['reps']:>6} {r['over_yardstick']:>12.3f} {r['byte_ratio']:>11.3f}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(dict(results=results), indent=1))
    sv.destroyComputeContext(ctx)
    return 0


if __name__ == "__main__":
    sys.exit(main())
