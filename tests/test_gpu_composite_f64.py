"""The tick kernels against the independent float64 statement of tests/composite_f64.py — directly, with no oracle in between.

Every other GPU test of these kernels compares with bytes of oracle/ref_kernels.c, written from the same reading of DESIGN.md section 4 as the
kernels; a misreading shared by both passes there.  Here every route a tick can take is FORCED (the `switch` fixture), its name asserted from
the batch's description, and the whole target — pre-filled with seeded bytes — is held to the statement's intervals: the cases of
tests/test_composite_f64.py (named, seeded, and the route shapes: no larger than the smallest at which a route is eligible and has more than
one strip, chunk or wave).  The float64 reference of a case is computed once and shared between the routes (test_composite_f64.statement).
One `f64:` line per compared plane: route, case, plane, the share of its bytes the statement leaves open (run with -s to see them)."""
import numpy as np
import pytest

import composite_f64 as F
import gpuutil as G
import test_composite_f64 as T
import util
from lanczos_f64 import assert_within
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv

pytestmark = pytest.mark.gpu

STREAM, WAVE, GENERAL = "tick_bgra_stream", "tick_bgra_wave", "tick_general_bgra"
STREAM_BATCHED = ["st-nv12-4", "st-nv12-2t", "st-y420p-3", "st-y420p-2t"]
STREAM_LONE = STREAM_BATCHED + ["st-nv12-1", "st-y420p-1"]
PHASED = [f"ph{t}" for t in range(5)]
BGRA_STRIPS = ["wv-mix", "wv-cover", "wv-metal"]
YUV_STREAMED = ["ys-nv12-video", "ys-y420p-video", "ys-nv12-int", "ys-y420p-int"]
YUV_STRIPS = YUV_STREAMED + ["yw-nv12-mix", "yw-y420p-mix"]


def float_rgb(name):
    """the case has a layer of the float RGB -> YUV kernels img_{bgra,rgba}_{nv12,y420p}: those cases have tests of their own below, one test
    per route and canvas format with the cases in a loop"""
    return any(F.KERNELS[layer[0]][2] == "premul" for layer in T.CASES[name][4])


# the float RGB -> YUV rows: float RGB layers only, a video layer under two of them (own | RGB kinds, three layers), all kinds in four layers
RGB_STREAMED = {fmt: [f"ys-{fmt}-{tick}" for tick in ("rgb", "rgb3", "all4")] for fmt in ("nv12", "y420p")}
RGB_STRIP_ONLY = {"nv12": "yw-nv12-premul", "y420p": "yw-y420p-premul"}
NAMED_BGRA = [n for n, c in T.NAMED.items() if c[0] == "bgra"]
NAMED_420 = [n for n, c in T.NAMED.items() if c[0] != "bgra" and not float_rgb(n)]
NAMED_RGB_420 = [n for n in T.NAMED if float_rgb(n)]
ODD_420 = ["odd-nv12", "odd-y420p", "odd-int"]
ODD_RGB_420 = ["odd-premul-nv12", "odd-premul-y420p"]
SINGLE, SINGLE_RGB = {}, {}                # kernel -> the named cases of one layer of it on a seeded canvas
for _n, _c in T.NAMED.items():
    if len(_c[4]) == 1 and _c[3] is not None:
        (SINGLE_RGB if float_rgb(_n) else SINGLE).setdefault(_c[4][0][0], []).append(_n)
USED = sorted(set(STREAM_LONE + PHASED + BGRA_STRIPS + YUV_STRIPS + sum(RGB_STREAMED.values(), []) + list(RGB_STRIP_ONLY.values())
                  + list(T.NAMED) + list(T.SEEDED) + list(T.SEEDED_PREMUL)))


def on_device(ctx, name):
    """(target, clear first, layers): the case's pictures uploaded; the target holds its seeded bytes whether the tick clears it or not"""
    fmt, W, H, canvas_seed, _ = T.CASES[name]
    planes, layers = T.build(name)
    dev = []
    for kernel, src, u, csc in layers:
        s = F.KERNELS[kernel][0]
        dev.append((sv.defaultComputeKernelFromString(kernel), G.to_gpu(ctx, s, src[0].shape[1], src[0].shape[0], util.copy_image(src)), u, csc))
    return G.to_gpu(ctx, fmt, W, H, util.copy_image(planes)), canvas_seed is None, dev


def held(ctx, route, name, target):
    fmt, W, H = T.CASES[name][:3]
    for i, ((lo, hi), got) in enumerate(zip(T.statement(name), G.from_gpu(ctx, target, fmt, W, H))):
        print(f"f64: {route}: {name} plane {i}: {100.0 * np.count_nonzero(lo != hi) / lo.size:.2f} % open")
        assert_within(lo, hi, got, f"{route}: {name} plane {i}")


def batched(ctx, names, expect):
    """the cases as one batch; `expect`: the route's name (None: whichever the library chooses)"""
    ticks = [on_device(ctx, n) for n in names]
    h, route, keep = G.make_batch(ctx, ticks)
    assert expect is None or route == expect, f"{names}: dispatched to {route}"
    G.run_batch(ctx, h)
    G.destroy_batch(h)
    for n, (target, _, _) in zip(names, ticks):
        held(ctx, route, n, target)
    return route


def lone(ctx, name, expect):
    """the case as a lone tick (chv_composite); the route is the one a batch of that tick describes"""
    target, clear, layers = on_device(ctx, name)
    h, route, keep = G.make_batch(ctx, [(target, clear, layers)])
    G.destroy_batch(h)
    assert route == expect, f"{name}: dispatched to {route}"
    sv.usingContext(ctx, lambda c: sv.compositeTick(c, target, layers, clear))
    held(ctx, route + ", lone", name, target)


# ---- BGRA canvases --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STREAM_BATCHED)
def test_stream_batched(ctx, switch, name):
    switch("CHV_BGRA_PATH", "stream")
    batched(ctx, [name], STREAM)


@pytest.mark.parametrize("name", STREAM_LONE)
def test_stream_lone(ctx, switch, name):
    switch("CHV_BGRA_PATH", "stream")
    lone(ctx, name, STREAM)


def test_stream_batch_planned_in_phases(ctx, switch):
    """five ticks cut into phases of falling chunk heights (CHV_STREAM_PLAN as tests/test_gpu_stream_plan.py sets it)"""
    switch("CHV_BGRA_PATH", "stream")
    switch("CHV_STREAM_PLAN", "40")
    before = cv.get_counter("stream_phased_launches")
    batched(ctx, PHASED, STREAM)
    assert cv.get_counter("stream_phased_launches") > before


@pytest.mark.parametrize("fmt", ["nv12", "y420p"])
def test_tiled(ctx, fmt):
    """one video layer per tick, batched: the single-purpose tiled kernels"""
    batched(ctx, [f"st-{fmt}-1"], f"tick_{fmt}_bgra_tiled")


@pytest.mark.parametrize("tables", ["tables", "in-place"])
@pytest.mark.parametrize("rows", ["8", "16"])
@pytest.mark.parametrize("name", BGRA_STRIPS + ["st-nv12-4"])
def test_bgra_strips(ctx, switch, name, rows, tables):
    """tick_bgra_wave at both strip heights, reading its geometry from tables (the session's CHV_GEOM_CACHE=eager) and computing it in place"""
    switch("CHV_BGRA_PATH", "wave")
    switch("CHV_WAVE_ROWS", rows)
    if tables == "in-place":
        switch("CHV_GEOM_CACHE", "0")
    batched(ctx, [name], WAVE)


@pytest.mark.parametrize("name", NAMED_BGRA + BGRA_STRIPS)
def test_general_bgra(ctx, switch, name):
    switch("CHV_FORCE_GENERAL", "1")
    batched(ctx, [name], GENERAL)


# ---- 4:2:0 canvases -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["batch", "lone"])
@pytest.mark.parametrize("name", YUV_STREAMED)
def test_yuv_stream(ctx, switch, name, how):
    """tick_yuv_stream: integer-matrix encoder layers and video layers, batched and as lone ticks"""
    switch("CHV_YUV_STREAM", "force")
    route = f"tick_yuv_stream<{T.CASES[name][0]}>"
    if how == "batch":
        batched(ctx, [name], route)
    else:
        lone(ctx, name, route)


@pytest.mark.parametrize("rows", ["8", "16"])
@pytest.mark.parametrize("name", YUV_STRIPS)
def test_yuv_strips(ctx, switch, name, rows):
    switch("CHV_YUV_STREAM", "0")
    switch("CHV_WAVE_ROWS", rows)
    batched(ctx, [name], f"tick_yuv_wave<{T.CASES[name][0]}>")


@pytest.mark.parametrize("name", ODD_420)
def test_odd_canvases_take_the_general_kernel(ctx, name):
    batched(ctx, [name], f"tick_general_yuv<{T.CASES[name][0]}>")


@pytest.mark.parametrize("name", NAMED_420 + YUV_STRIPS[-2:])
def test_general_yuv(ctx, switch, name):
    switch("CHV_FORCE_GENERAL", "1")
    batched(ctx, [name], f"tick_general_yuv<{T.CASES[name][0]}>")


# ---- 4:2:0 canvases, the float RGB -> YUV kernels: one test per route and canvas format, its cases in a loop -----------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "y420p"])
def test_yuv_stream_float_rgb(ctx, switch, fmt):
    """tick_yuv_stream's float RGB rows — float RGB layers only, the three-layer own | RGB instantiation, the all-kinds one — batched and lone"""
    switch("CHV_YUV_STREAM", "force")
    for name in RGB_STREAMED[fmt]:
        batched(ctx, [name], f"tick_yuv_stream<{fmt}>")
        lone(ctx, name, f"tick_yuv_stream<{fmt}>")


@pytest.mark.parametrize("fmt", ["nv12", "y420p"])
def test_yuv_strips_float_rgb(ctx, switch, fmt):
    """tick_yuv_wave at both strip heights on the same ticks and on the strip-only mix (border and fill, a flip, a layer across the left and top
    edges, a seeded canvas): the edge strips run the per-pixel statement, the interior the row code"""
    switch("CHV_YUV_STREAM", "0")
    for rows in ("8", "16"):
        switch("CHV_WAVE_ROWS", rows)
        for name in RGB_STREAMED[fmt] + [RGB_STRIP_ONLY[fmt]]:
            assert T.CASES[name][0] == fmt
            batched(ctx, [name], f"tick_yuv_wave<{fmt}>")


def test_general_yuv_float_rgb(ctx, switch):
    """tick_general_yuv: the odd canvases without a switch, then every named case and the strip-only mixes forced onto it"""
    for name in ODD_RGB_420:
        batched(ctx, [name], f"tick_general_yuv<{T.CASES[name][0]}>")
    switch("CHV_FORCE_GENERAL", "1")
    for name in NAMED_RGB_420 + list(RGB_STRIP_ONLY.values()):
        batched(ctx, [name], f"tick_general_yuv<{T.CASES[name][0]}>")


# ---- the single-kernel entry, the default routes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(SINGLE))
def test_run_compute_kernel_on_a_seeded_canvas(ctx, kernel):
    """every single-layer named case of one kernel through the single-kernel entry"""
    for name in SINGLE[kernel]:
        target, clear, ((k, src, u, csc),) = on_device(ctx, name)
        assert not clear and str(k) == kernel
        sv.usingContext(ctx, lambda c: sv.runComputeKernel(c, images=[src], target=target, kernel=k, uniforms=u, blends=True, colorspace=csc))
        held(ctx, "runComputeKernel", name, target)


@pytest.mark.parametrize("part", range(4))
def test_seeded_ticks_on_the_route_the_library_chooses(ctx, part):
    """a quarter of the seeded cases per test (every fourth one: all canvas formats in each), one batch per case"""
    for name in list(T.SEEDED)[part::4]:
        batched(ctx, [name], None)


def test_run_compute_kernel_float_rgb_on_a_seeded_canvas(ctx):
    """every single-layer named case of the four float RGB -> YUV kernels through the single-kernel entry"""
    assert len(SINGLE_RGB) == 4
    for kernel in sorted(SINGLE_RGB):
        for name in SINGLE_RGB[kernel]:
            target, clear, ((k, src, u, csc),) = on_device(ctx, name)
            assert not clear and str(k) == kernel
            sv.usingContext(ctx, lambda c: sv.runComputeKernel(c, images=[src], target=target, kernel=k, uniforms=u, blends=True, colorspace=csc))
            held(ctx, "runComputeKernel", name, target)


@pytest.mark.parametrize("part", range(2))
def test_seeded_float_rgb_ticks_on_the_route_the_library_chooses(ctx, part):
    """the seeded cases of the float RGB -> YUV kernels, sixteen per test (every second one: both canvas formats in each), one batch per case"""
    for name in list(T.SEEDED_PREMUL)[part::2]:
        batched(ctx, [name], None)


# ---- the caps, from the statement alone -----------------------------------------------------------------------------------------------------------
def test_caps_per_case_and_pooled():
    caps = F.Caps()
    for name in USED:
        caps.add(T.statement(name), name)
    caps.assert_pool("the cases of this module")
