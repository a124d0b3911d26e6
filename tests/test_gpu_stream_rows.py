"""tick_bgra_stream's row loop over chunks TALLER than its row table: small launches are cut into chunks of 4 - 12 canvas rows
(launch_bgra_stream), so only launches that fill the chip ever refill the table inside a chunk — here CHV_STREAM_ROWS forces the chunk
height, and every canvas is compared byte for byte with the oracle: chunk ends on both sides of a refill, every vertical ratio class the
kernel admits, pictures that start and end inside the canvas (rows outside the picture above, below and between refills), 2 - 4 layers of
NV12 and planar sources, as a batch and as a lone tick, a bottom layer of opacity exactly 1 and exactly 0."""
import pytest

import gpuutil as G
import util
from oracle import oracle as O
from swiftvideo_amd import compute as sv

pytestmark = pytest.mark.gpu

STREAM = "tick_bgra_stream"
HEIGHTS = [31, 32, 33, 64, 65, 720]
REDUCTIONS = [0.5, 1.0, 1.5, 2.0, 3.0, 4.0]
OPACITIES = [(1.0, 0.5, 0.25, 0.75), (0.0, 1.0, 0.5, 0.3), (0.6, 0.3, 1.0, 0.5), (1.0, 1.0, 0.4, 0.0)]
CHUNK_ROWS = [240, 33, 17, 64]              # canvas rows per chunk (the table holds 32 rows)


def _run(ctx, switch, cw, ch, fmt, sw, sh, ops, rows, seed, **kw):
    """one tick of len(ops) layers of one geometry through the streaming kernel with chunks of `rows` rows: as a batch, then as a lone tick"""
    switch("CHV_BGRA_PATH", "stream")
    switch("CHV_STREAM_ROWS", str(rows))
    exp = util.alloc_image("bgra", cw, ch)
    assert O.run_kernel("img_clear_bgra", exp) == 0
    layers = []
    for i, op in enumerate(ops):
        u = util.make_uniforms((cw, ch), in_size=(sw, sh), opacity=op, **kw)
        src = util.alloc_image(fmt, sw, sh, seed=seed + 7 * i)
        assert O.run_kernel(f"img_{fmt}_bgra", exp, src, u, csc=i % 4, threads=8) == 0
        layers.append((sv.defaultComputeKernelFromString(f"img_{fmt}_bgra"), G.to_gpu(ctx, fmt, sw, sh, src), u, i % 4))
    gd = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=seed + 99))
    h, name, keep = G.make_batch(ctx, [(gd, True, layers)])
    assert name == STREAM, f"dispatched to {name}"
    G.run_batch(ctx, h)
    G.destroy_batch(h)
    G.assert_same(G.from_gpu(ctx, gd, "bgra", cw, ch), exp, f"batch, chunks of {rows} rows")
    gd2 = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=seed + 98))
    sv.usingContext(ctx, lambda c: sv.compositeTick(c, gd2, layers, True))
    G.assert_same(G.from_gpu(ctx, gd2, "bgra", cw, ch), exp, f"lone tick, chunks of {rows} rows")


@pytest.mark.parametrize("red", REDUCTIONS)
@pytest.mark.parametrize("ch", HEIGHTS)
def test_full_canvas_rows(ctx, switch, ch, red):
    i = HEIGHTS.index(ch) * len(REDUCTIONS) + REDUCTIONS.index(red)
    nl, fmt = 2 + i % 3, ("nv12", "y420p")[(i // 3) % 2]
    sh = max(2, int(round(ch * red / 2)) * 2)
    _run(ctx, switch, 128, ch, fmt, 128, sh, OPACITIES[(i // 6 + i) % 4][:nl], CHUNK_ROWS[i % 4], seed=4000 + i)


INSIDE = [
    # canvas rows, (top, height) of the picture on the canvas, source rows, chunk rows
    (33, (5, 9), 14, 240),          # ends above the first refill
    (33, (10, 20), 30, 240),        # across the refill
    (65, (20, 40), 120, 240),       # starts between two refills, ends past the second; 3 : 1
    (65, (34, 25), 36, 33),         # a chunk of rows outside the picture, then one that starts above it
    (65, (-8, 50), 200, 17),        # starts above the canvas; 4 : 1
    (720, (100, 401), 602, 240),    # 1.5 : 1, chunks of 240 rows
    (720, (300, 200), 100, 64),     # enlarged
]


@pytest.mark.parametrize("case", range(len(INSIDE)))
def test_pictures_inside_the_canvas(ctx, switch, case):
    ch, (top, hh), sh, rows = INSIDE[case]
    nl, fmt = 2 + case % 3, ("y420p", "nv12")[case % 2]
    _run(ctx, switch, 128, ch, fmt, 128, sh, OPACITIES[case % 4][:nl], rows, seed=5000 + case, rect=(8, top, 112, hh))
