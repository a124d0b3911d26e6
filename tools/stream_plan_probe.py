"""tools/stream_plan_probe.py [canvas_w canvas_h src_w src_h ticks ...] — tick_bgra_stream's launch plan on shapes bench.py has no workload for:
a batch of `ticks` four-layer NV12 ticks (opacity 1 / .75 / .5 / .25, the headline's tick) onto canvases of the given size, timed between two
events with CHV_STREAM_PLAN=1 and =0 alternating in ONE process (the switch goes through chv_debug_set_switch).  Prints the medians of
`rounds` x `reps` launches per setting and whether the launch was phased.  Run on the GPU box.  Default: 1920x1080 canvases from 1920x1080
sources at 16, 32, 64 and 96 ticks."""
import ctypes as C
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import gpuutil as G
import util
from swiftvideo_amd import chipvideo as cv, compute as sv

args = [int(a) for a in sys.argv[1:]] or [1920, 1080, 1920, 1080, 16, 32, 64, 96]
cw, ch, sw, sh, counts = args[0], args[1], args[2], args[3], args[4:]
ROUNDS, REPS = 5, 40
ctx = sv.makeComputeContext(forType="GPU")
lib = cv.load()
cv.set_switch("CHV_BGRA_PATH", "stream")
e0, e1 = C.c_void_p(), C.c_void_p()
cv.check(lib.chv_event_create(ctx.handle, C.byref(e0))); cv.check(lib.chv_event_create(ctx.handle, C.byref(e1)))
srcs = [G.to_gpu(ctx, "nv12", sw, sh, util.alloc_image("nv12", sw, sh, seed=2 + i)) for i in range(4)]
k = sv.defaultComputeKernelFromString("img_nv12_bgra")
for n in counts:
    ticks = []
    for t in range(n):
        layers = [(k, srcs[(t + i) % 4], util.make_uniforms((cw, ch), in_size=(sw, sh), opacity=op), 0) for i, op in enumerate((1.0, 0.75, 0.5, 0.25))]
        ticks.append((G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch)), True, layers))
    h, name, keep = G.make_batch(ctx, ticks)
    ms = {"1": [], "0": []}
    phased = {}
    for rnd in range(ROUNDS + 1):                       # (round 0: warm-up)
        for plan in ("1", "0"):
            cv.set_switch("CHV_STREAM_PLAN", plan)
            before = cv.get_counter("stream_phased_launches")
            for _ in range(REPS):
                lib.chv_event_record(ctx.handle, e0)
                cv.check(lib.chv_batch_run(ctx.handle, h))
                lib.chv_event_record(ctx.handle, e1)
                cv.check(lib.chv_pass_end(ctx.handle, 1))
                v = C.c_float(); lib.chv_event_elapsed_ms(e0, e1, C.byref(v))
                if rnd:
                    ms[plan].append(v.value)
            phased[plan] = cv.get_counter("stream_phased_launches") > before
    m1, m0 = statistics.median(ms["1"]), statistics.median(ms["0"])
    print(f"{n} ticks {sw}x{sh} -> {cw}x{ch} kernel {name}: CHV_STREAM_PLAN=1 {'phased' if phased['1'] else 'uniform'} median {m1:.4f} ms "
          f"(min {min(ms['1']):.4f}), =0 median {m0:.4f} ms (min {min(ms['0']):.4f}), ratio {m1 / m0:.4f}", flush=True)
    G.destroy_batch(h)
    del ticks, keep
cv.set_switch("CHV_STREAM_PLAN", None)
sv.destroyComputeContext(ctx)
