"""The chroma-carry kernels of tick_bgra_stream (kernels_stream_carry.hip.cpp: tick_bgra_stream_cc).  launch_bgra_stream_opaque sends a launch
there when it is an NV12 batch (not the by-value lone tick), CHV_STREAM_CARRY is on and the chroma plane advances by at most one row per
canvas row (stream_select.h); the lane then keeps the chroma bytes of the two ring rows it taps and reads only the rows that are new to it.
Every canvas here is compared byte for byte with the oracle, first through the new kernels (`stream_carry_launches` AND
`stream_opaque_launches` must move), then with CHV_STREAM_CARRY=0 through tick_bgra_stream_ob (the carry counter must not move, the
opaque one still does): the same bytes from both.

The shapes put every state of the carry on a small canvas — advance 0 (nothing read), advance 1 (one parity read), the chunk's first row and
larger advances (both read) — and every shape runs with forced chunk heights 4, 13, 52 and 64: chunk starts at every parity of the chroma
row, on both sides of the row table's 32 rows.  2, 3 and 4 layers, the three absorbed matrices mixed across layers, three opacity sets.

Two notes on the shapes.  321x52 <- 480x208 was specified as "exactly one chroma row per canvas row", but its chroma plane (104 rows) advances
TWO rows per canvas row: it stays, the predicate declines it (and the bytes must match); the shape whose chroma advances exactly one row
per canvas row — the predicate's boundary, which it takes — is 321x52 <- 480x104 and stands beside it.  The odd source height (480x105)
has the chroma height of this project's plane table, h // 2 = 52 rows (compute.py: planesForFormat, after the reference's), not
(h + 1) / 2.
Fixed seeds; nothing is skipped."""
import numpy as np
import pytest

import gpuutil as G
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv

pytestmark = pytest.mark.gpu

STREAM = "tick_bgra_stream"
CARRY, OPAQUE = "stream_carry_launches", "stream_opaque_launches"
BT601_FULL = 2                               # the one matrix without absorbing biases
GEOMETRIES = [
    # canvas, source, rectangle of the picture on the canvas (None: the whole canvas), the predicate's answer (chroma rows per canvas row)
    ((321, 70), (480, 104), None, True),                 # the headline's class: 52 / 70, chroma advances 1, 1, 1, 0
    ((321, 70), (160, 36), None, True),                  # enlarged: 18 / 70, long runs of advance 0; the clamped last chroma row
    ((321, 52), (480, 208), None, False),                # 104 / 52 = 2: both sets read on every row
    ((321, 52), (480, 104), None, True),                 # 52 / 52 = 1 exactly: the predicate's boundary, advance 1 on every row
    ((283, 33), (480, 130), None, False),                # 4 : 1 down: 65 / 33
    ((321, 70), (320, 90), (40, 5, 200, 60), True),      # rows and columns outside the picture: 45 chroma rows over 60 canvas rows
    ((321, 70), (480, 105), None, True),                 # an odd source height: 52 / 70
]
OPACITIES = [(1.0, 0.75, 0.5, 0.25), (1.0, 0.0, 1.0, 0.3), (1.0, 1.0, 0.0, 0.6)]
CHUNK_ROWS = [4, 13, 52, 64]
ABSORBED = [0, 1, 3]


def _cleared(cw, ch):
    exp = util.alloc_image("bgra", cw, ch)
    assert O.run_kernel("img_clear_bgra", exp) == 0
    return exp


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


def _run_batch(ctx, ticks, exps, want_carry, want_opaque, what):
    c0, o0 = cv.get_counter(CARRY), cv.get_counter(OPAQUE)
    h, name, keep = G.make_batch(ctx, ticks)
    assert name == STREAM, f"dispatched to {name}"
    G.run_batch(ctx, h)
    G.destroy_batch(h)
    assert (cv.get_counter(CARRY) > c0) == want_carry, (what, "carry counter", c0, cv.get_counter(CARRY))
    assert (cv.get_counter(OPAQUE) > o0) == want_opaque, (what, "opaque counter", o0, cv.get_counter(OPAQUE))
    for t, (gd, _, _) in enumerate(ticks):
        cw, ch = exps[t][0].shape[1], exps[t][0].shape[0]
        G.assert_same(G.from_gpu(ctx, gd, "bgra", cw, ch), exps[t], f"tick {t}, {what}")


def _both_routes(ctx, switch, canvas, fmt, src_size, ops, cscs, rows, seed, rect=None, carry=True, opaque=True, n_ticks=1):
    """a batch through the chroma-carry kernels (where `carry`) and, with CHV_STREAM_CARRY=0, through the kernels they replace; then the
    first tick as a lone tick, which never takes them"""
    cw, ch = canvas
    switch("CHV_BGRA_PATH", "stream")
    switch("CHV_STREAM_ROWS", str(rows))
    exps, tick_layers = [], []
    for t in range(n_ticks):
        exp = _cleared(cw, ch)
        tick_layers.append(_layers(ctx, exp, canvas, fmt, src_size, ops if t == 0 else (ops[0],) + tuple(0.15 + 0.2 * t + 0.1 * i for i in range(len(ops) - 1)),
                                   cscs, seed + 31 * t, rect))
        exps.append(exp)
    for enabled in ("1", "0"):
        switch("CHV_STREAM_CARRY", enabled)
        what = f"CHV_STREAM_CARRY={enabled}, chunks of {rows} rows"
        ticks = [(G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=seed + 90 + t)), True, tick_layers[t]) for t in range(n_ticks)]
        _run_batch(ctx, ticks, exps, carry and enabled == "1", opaque, what)
    switch("CHV_STREAM_CARRY", "1")
    c0 = cv.get_counter(CARRY)
    gd = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=seed + 98))
    sv.usingContext(ctx, lambda c: sv.compositeTick(c, gd, tick_layers[0], True))
    assert cv.get_counter(CARRY) == c0, "a lone tick took the chroma-carry kernels"
    G.assert_same(G.from_gpu(ctx, gd, "bgra", cw, ch), exps[0], f"lone tick, chunks of {rows} rows")


@pytest.mark.parametrize("rows", CHUNK_ROWS)
@pytest.mark.parametrize("geom", range(len(GEOMETRIES)))
def test_carry_matches_oracle_and_transient_kernels(ctx, switch, geom, rows):
    canvas, src_size, rect, carry = GEOMETRIES[geom]
    i = geom * len(CHUNK_ROWS) + CHUNK_ROWS.index(rows)
    nl = 2 + i % 3                                        # (four chunk heights per shape: every shape sees 2, 3 and 4 layers)
    cscs = [ABSORBED[(i + l) % 3] for l in range(nl)]
    _both_routes(ctx, switch, canvas, "nv12", src_size, OPACITIES[(i // 3) % 3][:nl], cscs, rows, seed=9000 + 13 * i, rect=rect, carry=carry)


@pytest.mark.parametrize("ops", range(len(OPACITIES)))
@pytest.mark.parametrize("nl", [2, 3, 4])
def test_every_layer_count_and_opacity_set_on_the_headline_shape(ctx, switch, nl, ops):
    _both_routes(ctx, switch, (321, 70), "nv12", (480, 104), OPACITIES[ops][:nl], [ABSORBED[(ops + l) % 3] for l in range(nl)], 13, seed=9500 + 10 * nl + ops)


def test_a_batch_of_three_ticks_with_different_sources(ctx, switch):
    _both_routes(ctx, switch, (321, 70), "nv12", (480, 104), OPACITIES[0], [0, 1, 3, 0], 13, seed=9600, n_ticks=3)


def test_a_planar_launch_keeps_the_transient_kernels(ctx, switch):
    _both_routes(ctx, switch, (321, 70), "y420p", (480, 104), OPACITIES[0], [0, 1, 3, 0], 13, seed=9700, carry=False)


def test_a_bottom_layer_that_is_not_exactly_opaque_keeps_the_general_kernels(ctx, switch):
    _both_routes(ctx, switch, (321, 70), "nv12", (480, 104), (float(np.float32(0.99999994)), 0.6, 0.3), [0, 1, 3], 13, seed=9710, carry=False, opaque=False)


def test_a_plain_matrix_layer_keeps_the_general_kernels(ctx, switch):
    _both_routes(ctx, switch, (321, 70), "nv12", (480, 104), (1.0, 0.6, 0.3), [0, BT601_FULL, 1], 13, seed=9720, carry=False, opaque=False)


def test_a_lone_tick_keeps_the_transient_kernels(ctx, switch):
    """the by-value lone tick (tick_bgra_stream_ob_one) on the headline's shape: the opaque counter moves, the carry counter does not"""
    switch("CHV_BGRA_PATH", "stream")
    switch("CHV_STREAM_ROWS", "13")
    cw, ch = 321, 70
    exp = _cleared(cw, ch)
    layers = _layers(ctx, exp, (cw, ch), "nv12", (480, 104), OPACITIES[0], [0, 1, 3, 0], 9730, None)
    c0, o0 = cv.get_counter(CARRY), cv.get_counter(OPAQUE)
    gd = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=9739))
    sv.usingContext(ctx, lambda c: sv.compositeTick(c, gd, layers, True))
    assert cv.get_counter(CARRY) == c0 and cv.get_counter(OPAQUE) > o0
    G.assert_same(G.from_gpu(ctx, gd, "bgra", cw, ch), exp, "lone tick")
