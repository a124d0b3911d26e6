"""The opaque-bottom kernels of tick_bgra_stream (kernels_stream_opq.hip.cpp: tick_bgra_stream_ob, and tick_bgra_stream_ob_one for lone ticks).
launch_bgra_stream takes them when every tick's bottom layer has opacity exactly 1, there are two layers or more and every layer's colour
matrix has an absorbed form; the bottom layer then computes no blend and layer 1 takes its code through one fused multiply-add.  Every canvas
here is compared byte for byte with the oracle, first through the new kernels (the library's counter `stream_opaque_launches` must move),
then with CHV_STREAM_OPAQUE=0 through the kernels they replace (the counter must not move): the same bytes from both.

2 - 4 layers of NV12 and planar sources, every colour matrix (a launch with a BT.601 full-range layer has no absorbed form: it keeps the
general kernels, and stays exact), reductions of 1.5 : 1, an enlargement, 1.7 : 1 across with 4 : 1 down, odd canvas widths (lanes beyond
the canvas), a picture inside the canvas (columns left and right of it keep the cleared word; its source is tapped from its first to
its last column), forced chunk heights on both sides of the row table's 32 rows, batches and lone ticks, upper-layer
opacities that include 0 and 1.  Fixed seeds; nothing is skipped."""
import numpy as np
import pytest

import gpuutil as G
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv

pytestmark = pytest.mark.gpu

STREAM = "tick_bgra_stream"
COUNTER = "stream_opaque_launches"
BT601_FULL = 2                               # the one matrix without absorbing biases (pixel_math.hip.h: csc_absorbable)
GEOMETRIES = [
    # canvas, source, rectangle of the picture on the canvas (None: the whole canvas)
    ((321, 70), (480, 104), None),           # 1.5 : 1
    ((321, 70), (160, 36), None),            # enlarged 2 x
    ((283, 33), (480, 130), None),           # 1.7 : 1 across, 4 : 1 down
    ((321, 70), (320, 90), (40, 5, 200, 60)),    # a picture inside the canvas: canvas columns 40 .. 239, rows 5 .. 64
]
OPACITIES = [(1.0, 0.75, 0.5, 0.25), (1.0, 0.0, 1.0, 0.3), (1.0, 1.0, 0.0, 0.6), (1.0, 0.5, 1.0, 0.0)]
CHUNK_ROWS = [4, 13, 52, 64]
ABSORBED = [0, 1, 3]


def _layers(ctx, exp, canvas, fmt, src_size, ops, cscs, seed, rect):
    """the layers of one tick, applied to `exp` by the oracle on the way"""
    (cw, ch), (sw, sh) = canvas, src_size
    layers = []
    for i, (op, csc) in enumerate(zip(ops, cscs)):
        u = util.make_uniforms((cw, ch), in_size=(sw, sh), opacity=op, **({"rect": rect} if rect else {}))
        src = util.alloc_image(fmt, sw, sh, seed=seed + 7 * i)
        assert O.run_kernel(f"img_{fmt}_bgra", exp, src, u, csc=csc, threads=8) == 0
        layers.append((sv.defaultComputeKernelFromString(f"img_{fmt}_bgra"), G.to_gpu(ctx, fmt, sw, sh, src), u, csc))
    return layers


def _cleared(cw, ch):
    exp = util.alloc_image("bgra", cw, ch)
    assert O.run_kernel("img_clear_bgra", exp) == 0
    return exp


def _both_routes(ctx, switch, canvas, fmt, src_size, ops, cscs, rows, seed, rect=None, opaque_form=True):
    """one tick as a batch and as a lone tick, through the opaque-bottom kernels (where `opaque_form`) and through the general ones"""
    cw, ch = canvas
    switch("CHV_BGRA_PATH", "stream")
    switch("CHV_STREAM_ROWS", str(rows))
    exp = _cleared(cw, ch)
    layers = _layers(ctx, exp, canvas, fmt, src_size, ops, cscs, seed, rect)
    for enabled in ("1", "0"):
        switch("CHV_STREAM_OPAQUE", enabled)
        what = f"CHV_STREAM_OPAQUE={enabled}, chunks of {rows} rows"
        want_new = opaque_form and enabled == "1"
        c0 = cv.get_counter(COUNTER)
        gd = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=seed + 99))
        h, name, keep = G.make_batch(ctx, [(gd, True, layers)])
        assert name == STREAM, f"dispatched to {name}"
        G.run_batch(ctx, h)
        G.destroy_batch(h)
        c1 = cv.get_counter(COUNTER)
        assert (c1 > c0) == want_new, (what, "batch", c0, c1)
        G.assert_same(G.from_gpu(ctx, gd, "bgra", cw, ch), exp, "batch, " + what)
        gd2 = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=seed + 98))
        sv.usingContext(ctx, lambda c: sv.compositeTick(c, gd2, layers, True))
        c2 = cv.get_counter(COUNTER)
        assert (c2 > c1) == want_new, (what, "lone tick", c1, c2)
        G.assert_same(G.from_gpu(ctx, gd2, "bgra", cw, ch), exp, "lone tick, " + what)


@pytest.mark.parametrize("nl", [2, 3, 4])
@pytest.mark.parametrize("fmt", ["nv12", "y420p"])
@pytest.mark.parametrize("geom", range(len(GEOMETRIES)))
def test_opaque_bottom_matches_oracle_and_general_kernels(ctx, switch, geom, fmt, nl):
    canvas, src_size, rect = GEOMETRIES[geom]
    i = (geom * 2 + ("nv12", "y420p").index(fmt)) * 3 + nl - 2
    cscs = [ABSORBED[(i + l) % 3] for l in range(nl)]
    _both_routes(ctx, switch, canvas, fmt, src_size, OPACITIES[i % 4][:nl], cscs, CHUNK_ROWS[(i // 2) % 4], seed=7000 + i, rect=rect)


@pytest.mark.parametrize("rows", CHUNK_ROWS)
def test_every_chunk_height_on_the_headline_shape(ctx, switch, rows):
    """four NV12 layers at 1.5 : 1, opacities 1 / .75 / .5 / .25 (the bench headline's tick in small)"""
    _both_routes(ctx, switch, (321, 70), "nv12", (480, 104), OPACITIES[0], [0, 1, 3, 0], rows, seed=7100 + rows)


@pytest.mark.parametrize("fmt", ["nv12", "y420p"])
@pytest.mark.parametrize("csc", [0, 1, 2, 3])
def test_every_colour_matrix(ctx, switch, csc, fmt):
    """all layers of one matrix; BT.601 full range has no absorbed form, so its launches keep the general kernels (plain matrix)"""
    _both_routes(ctx, switch, (193, 40), fmt, (288, 60), (1.0, 0.6, 0.3), [csc] * 3, 13, seed=7200 + csc, opaque_form=csc != BT601_FULL)


def test_one_plain_matrix_layer_keeps_the_general_kernels(ctx, switch):
    _both_routes(ctx, switch, (193, 40), "nv12", (288, 60), (1.0, 0.6, 0.3), [0, BT601_FULL, 1], 52, seed=7300, opaque_form=False)


@pytest.mark.parametrize("bottom", [np.float32(0.99999994), 0.5, 0.0])
def test_a_bottom_layer_that_is_not_exactly_opaque_keeps_the_general_kernels(ctx, switch, bottom):
    _both_routes(ctx, switch, (193, 40), "nv12", (288, 60), (float(bottom), 0.6, 0.3), [0, 1, 3], 13, seed=7400, opaque_form=False)


def test_a_single_layer_keeps_the_general_kernels(ctx, switch):
    _both_routes(ctx, switch, (193, 40), "nv12", (288, 60), (1.0,), [0], 13, seed=7500, opaque_form=False)


@pytest.mark.parametrize("odd_one", [None, 1])
def test_batches_of_several_ticks(ctx, switch, odd_one):
    """three ticks in one launch: the opaque-bottom kernels only when EVERY tick's bottom layer is opaque"""
    switch("CHV_BGRA_PATH", "stream")
    switch("CHV_STREAM_ROWS", "13")
    (cw, ch), src_size = (321, 70), (480, 104)
    ticks, exps = [], []
    for t in range(3):
        ops = (0.99999994 if t == odd_one else 1.0, 0.4 + 0.1 * t, 0.25)
        exp = _cleared(cw, ch)
        layers = _layers(ctx, exp, (cw, ch), "nv12", src_size, ops, [0, 1, 3], 7600 + 31 * t, None)
        ticks.append((G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=7690 + t)), True, layers))
        exps.append(exp)
    for enabled in ("1", "0"):
        switch("CHV_STREAM_OPAQUE", enabled)
        c0 = cv.get_counter(COUNTER)
        h, name, keep = G.make_batch(ctx, ticks)
        assert name == STREAM, f"dispatched to {name}"
        G.run_batch(ctx, h)
        G.destroy_batch(h)
        assert (cv.get_counter(COUNTER) > c0) == (enabled == "1" and odd_one is None)
        for t, (gd, _, _) in enumerate(ticks):
            G.assert_same(G.from_gpu(ctx, gd, "bgra", cw, ch), exps[t], f"tick {t}, CHV_STREAM_OPAQUE={enabled}")
