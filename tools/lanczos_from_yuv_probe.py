"""tools/lanczos_from_yuv_probe.py [--yardstick] [--against yardstick.json] [--runs 15] [--window-ms 20] [--out file.json] — device time of
chv_scale_lanczos_from_yuv / chv_scale_lanczos_from_yuv_batch (NV12 or y420p -> BGRA with Lanczos-3 in one launch) and of the only route the
PARENT commit offers for the pair: a same-size full-canvas img_nv12_bgra / img_y420p_bgra tick into a BGRA intermediate followed by
chv_scale_lanczos / chv_scale_lanczos_batch to the target size.  That chain's bytes differ (its first step is a bilinear sampler, not this
specification): a time comparison only.

  geometries  1920x1080 -> 1280x720, 3840x2160 -> 1920x1080; both packings; 1 picture and 16

A process measures one library.  Without --yardstick it is the tree's own: the new entries, and as context chv_scale_lanczos_420 /
chv_scale_lanczos_420_ladder (one rung) into the other packing for the same sizes — the same luma work, less chroma work, 1.5 instead of 4
bytes a pixel written.  With --yardstick the library is the one CHV_LIB names — the parent's, which does not have the new entries: the binding
is loaded without them and the two-launch chain is measured TWICE, as sides `chain` and `chain_again` of the same run (an A/A pair: what the
probe itself cannot tell apart).  Never the new code as its own yardstick.  --against reads a yardstick's --out file and prints the new
entry's time over the chain's and THE CONDITION: the single call is not slower than the chain beyond the chain's A/A difference (exit status 1).

Every call of a window works on buffers of its own, rotated call by call, so that no call finds its source in the Infinity Cache because the
call before it read it.  A window holds nothing but C calls through ctypes with arguments made beforehand, between two chv_event records; its
length is chosen per side so that it lasts about --window-ms; every side is warmed up first and the sides alternate window by window.  A time
is the median over --runs windows, in microseconds per call (a call of 16 pictures counts once); `spread` is (max - min) / median of a side's
windows.  Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

GEOMETRIES = [((1920, 1080), (1280, 720)), ((3840, 2160), (1920, 1080))]
FORMATS = ["nv12", "y420p"]
SETS = 32                   # pictures per (geometry, format): 32 lone calls or two lists of 16 before a buffer comes round again
NEW = ("chv_scale_lanczos_from_yuv", "chv_scale_lanczos_from_yuv_batch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--against", default=None)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from swiftvideo_amd import chipvideo as cv
    if a.yardstick:
        for name in NEW:
            cv._SIGNATURES.pop(name)
    import numpy as np
    import gpuutil as G
    import util
    from swiftvideo_amd import compute as sv
    lib = cv.load()
    ctx = sv.makeComputeContext(forType="GPU")
    handle = ctx.handle
    K = sv.defaultComputeKernelFromString

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

    sides, keep = {}, []
    for (iw, ih), (ow, oh) in GEOMETRIES:
        geo = f"{iw}x{ih}->{ow}x{oh}"
        targets = [G.to_gpu(ctx, "bgra", ow, oh, util.alloc_image("bgra", ow, oh)) for _ in range(SETS)]
        t_img = images(targets)
        keep += [targets, t_img]
        mids = [G.to_gpu(ctx, "bgra", iw, ih, util.alloc_image("bgra", iw, ih)) for _ in range(SETS)] if a.yardstick else []
        m_img = images(mids) if mids else None
        keep += [mids, m_img]
        for fmt in FORMATS:
            host = util.alloc_image(fmt, iw, ih, seed=1)
            srcs = [G.to_gpu(ctx, fmt, iw, ih, host) for _ in range(SETS)]
            s_img = images(srcs)
            keep += [srcs, s_img]
            groups = SETS // 16
            if a.yardstick:
                quad = sv._unit_quad_to_ndc()
                layers, ticks = [], []
                for k in range(SETS):
                    full = srcs[k].derive(matrix=quad, textureMatrix=np.eye(4), borderMatrix=quad, fillColor=(0.0, 0.0, 0.0, 0.0), opacity=1.0)
                    layer = (K(f"img_{fmt}_bgra"), full, sv.imageUniformsFor(full, mids[k]), cv.CSC_BT601_LIMITED)
                    layers.append(sv._layer_array([layer]))
                    ticks.append((mids[k], True, [layer]))
                batches = [sv.TickBatch(ctx, ticks[16 * j: 16 * j + 16]) for j in range(groups)]
                keep += [layers, ticks, batches]

                def chain1(k, layers=layers, m_img=m_img, t_img=t_img):
                    k %= SETS
                    if lib.chv_composite(handle, C.byref(m_img[k]), 1, layers[k], 1) or lib.chv_scale_lanczos(handle, C.byref(t_img[k]), C.byref(m_img[k])):
                        raise RuntimeError("the chain of one picture failed")

                def chain16(k, batches=batches, m_img=m_img, t_img=t_img):
                    j = k % groups
                    if lib.chv_batch_run(handle, batches[j]._h) or \
                            lib.chv_scale_lanczos_batch(handle, C.byref(t_img, 16 * j * C.sizeof(cv.Image)), C.byref(m_img, 16 * j * C.sizeof(cv.Image)), 16):
                        raise RuntimeError("the chain of 16 pictures failed")
                for name in ("chain", "chain_again"):
                    sides[(geo, fmt, 1, name)] = chain1
                    sides[(geo, fmt, 16, name)] = chain16
            else:
                other = "y420p" if fmt == "nv12" else "nv12"
                yuv = [G.to_gpu(ctx, other, ow, oh, util.alloc_image(other, ow, oh)) for _ in range(SETS)]
                y_img = images(yuv)
                opts = cv.KernelOpts(colorspace=cv.CSC_BT601_LIMITED)
                keep += [yuv, y_img, opts]

                def new1(k, s_img=s_img, t_img=t_img, opts=opts):
                    k %= SETS
                    if lib.chv_scale_lanczos_from_yuv(handle, C.byref(t_img[k]), C.byref(s_img[k]), C.byref(opts)):
                        raise RuntimeError("the single call failed")

                def new16(k, s_img=s_img, t_img=t_img, opts=opts):
                    off = 16 * (k % groups) * C.sizeof(cv.Image)
                    if lib.chv_scale_lanczos_from_yuv_batch(handle, C.byref(t_img, off), C.byref(s_img, off), 16, C.byref(opts)):
                        raise RuntimeError("the list of 16 pictures failed")

                def x1(k, s_img=s_img, y_img=y_img):
                    k %= SETS
                    if lib.chv_scale_lanczos_420(handle, C.byref(y_img[k]), C.byref(s_img[k])):
                        raise RuntimeError("chv_scale_lanczos_420 failed")

                def x16(k, s_img=s_img, y_img=y_img):
                    off = 16 * (k % groups) * C.sizeof(cv.Image)
                    if lib.chv_scale_lanczos_420_ladder(handle, C.byref(y_img, off), 1, C.byref(s_img, off), 16):
                        raise RuntimeError("chv_scale_lanczos_420_ladder failed")
                sides[(geo, fmt, 1, "from_yuv")], sides[(geo, fmt, 16, "from_yuv")] = new1, new16
                sides[(geo, fmt, 1, "to_other_420")], sides[(geo, fmt, 16, "to_other_420")] = x1, x16

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
    for (geo, fmt, n, side), t in times.items():
        med = statistics.median(t)
        results.append(dict(geometry=geo, format=fmt, pictures=n, side=side, us=round(med, 2), spread=round((max(t) - min(t)) / med, 4),
                            reps=reps[(geo, fmt, n, side)], runs=a.runs))
    what = "yardstick (the library CHV_LIB names: composite tick + chv_scale_lanczos, measured twice)" if a.yardstick else "the tree's library"
    print(f"# {what}; build flags: {cv.build_flags()}")
    print(f"{'geometry':>22} {'format':>6} {'n':>3} {'side':>13} {'us':>10} {'spread':>7} {'reps':>5}")
    for r in results:
        print(f"{r['geometry']:>22} {r['format']:>6} {r['pictures']:>3} {r['side']:>13} {r['us']:>10.2f} {r['spread']:>7.4f} {r['reps']:>5}")
    ok = True
    if a.against:
        base = {(r["geometry"], r["format"], r["pictures"], r["side"]): r["us"] for r in json.loads(Path(a.against).read_text())["results"]}
        print(f"{'geometry':>22} {'format':>6} {'n':>3} {'from_yuv us':>12} {'chain us':>10} {'ratio':>7} {'A/A':>7} {'to_other_420 us':>16}")
        for r in results:
            if r["side"] != "from_yuv":
                continue
            key = (r["geometry"], r["format"], r["pictures"])
            ch, again = base[key + ("chain",)], base[key + ("chain_again",)]
            aa = abs(ch - again) / min(ch, again)
            r["chain_us"], r["over_chain"], r["chain_aa"] = ch, round(r["us"] / ch, 4), round(aa, 4)
            ctx_us = next(x["us"] for x in results if x["side"] == "to_other_420" and (x["geometry"], x["format"], x["pictures"]) == key)
            miss = r["us"] > max(ch, again) * (1 + aa)
            ok = ok and not miss
            print(f"{r['geometry']:>22} {r['format']:>6} {r['pictures']:>3} {r['us']:>12.2f} {ch:>10.2f} {r['over_chain']:>7.3f} {aa:>7.4f} {ctx_us:>16.2f}{'  MISSED' if miss else ''}")
        print("condition: " + ("met" if ok else "MISSED") + " (the single call is not slower than the two-launch chain beyond the chain's A/A difference)")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(dict(yardstick=a.yardstick, results=results, condition=ok), indent=1))
    sv.destroyComputeContext(ctx)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
