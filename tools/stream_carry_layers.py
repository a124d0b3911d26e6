"""tools/stream_carry_layers.py [ticks] — the chroma-carry kernels of tick_bgra_stream (kernels_stream_carry.hip.cpp) against the kernels they
replace (CHV_STREAM_CARRY=0), per layer count and vertical ratio, in ONE process on one card: batches of `ticks` (default 48) ticks of 2 / 3 / 4
NV12 layers with an opaque bottom onto 720p BGRA canvases — 1080p sources (0.75 chroma rows per canvas row, the headline's class), 720p
sources (0.5) and 1920x1440 sources (exactly 1, the predicate's boundary); every tick has sources and a canvas of its own.  Five alternating
rounds, each 40 launches back to back between two stream events; ms per launch and the ratio of the medians.  GPU box.
(profiles/stream_chroma_carry_notes.md section 6.)"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import ctypes as C
import numpy as np
import util, gpuutil as G
from swiftvideo_amd import compute as sv, chipvideo as cv

TICKS = int(sys.argv[1]) if len(sys.argv) > 1 else 48
ctx = sv.makeComputeContext(forType="GPU")
lib = cv.load()
e0, e1 = C.c_void_p(), C.c_void_p()
cv.check(lib.chv_event_create(ctx.handle, C.byref(e0))); cv.check(lib.chv_event_create(ctx.handle, C.byref(e1)))
K = sv.defaultComputeKernelFromString("img_nv12_bgra")
CW, CH = 1280, 720
rng = np.random.default_rng(11)


def launch_ms(h, n=40):
    """ms per launch of `n` launches issued back to back between two stream events (as bench.py times a workload)"""
    cv.check(lib.chv_event_record(ctx.handle, e0))
    for _ in range(n):
        cv.check(lib.chv_batch_run(ctx.handle, h))
    cv.check(lib.chv_event_record(ctx.handle, e1))
    cv.check(lib.chv_pass_end(ctx.handle, 1))
    ms = C.c_float(); cv.check(lib.chv_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value / n


for (sw, sh) in ((1920, 1080), (1280, 720), (1920, 1440)):
    planes = [rng.integers(0, 256, p.shape, dtype=np.uint8) for p in util.alloc_image("nv12", sw, sh)]
    for nl in (2, 3, 4):
        ticks = []
        for t in range(TICKS):
            layers = [(K, G.to_gpu(ctx, "nv12", sw, sh, planes), util.full_canvas_uniforms((CW, CH), (sw, sh), opacity=(1.0, 0.75, 0.5, 0.25)[l]), 0) for l in range(nl)]
            ticks.append((G.to_gpu(ctx, "bgra", CW, CH, util.alloc_image("bgra", CW, CH)), True, layers))
        res = {"1": [], "0": []}
        for rnd in range(5):
            for carry in ("1", "0"):
                cv.set_switch("CHV_STREAM_CARRY", carry)
                c0 = cv.get_counter("stream_carry_launches")
                h, name, keep = G.make_batch(ctx, ticks)
                launch_ms(h, 5)
                res[carry].append(launch_ms(h))
                took = cv.get_counter("stream_carry_launches") > c0
                G.destroy_batch(h)
                assert name == "tick_bgra_stream" and took == (carry == "1"), (name, took, carry)
        cv.set_switch("CHV_STREAM_CARRY", None)
        a, b = np.median(res["1"]), np.median(res["0"])
        print(f"{sw}x{sh} -> {CW}x{CH}, {nl} layers, {TICKS} ticks: carry {min(res['1']):.4f} - {max(res['1']):.4f} ms, transient {min(res['0']):.4f} - {max(res['0']):.4f} ms, "
              f"median ratio {a / b:.3f}", flush=True)
        del ticks
