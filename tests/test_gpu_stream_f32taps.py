"""The f32-tap kernels of tick_bgra_stream (kernels_stream_dn.hip.cpp: tick_bgra_stream_cd).  launch_bgra_stream_opaque sends every launch the
chroma-carry kernels take there while CHV_STREAM_F32TAPS is on: the tap bytes enter v_fma_f32 / v_fmac_f32 as binary32 denormals instead of
v_fma_mix_f32 as binary16 ones.  Every canvas here is compared byte for byte with the oracle, first through the new kernels
(`stream_f32tap_launches`, `stream_carry_launches` AND `stream_opaque_launches` must move), then with CHV_STREAM_F32TAPS=0 through
tick_bgra_stream_cc (the new counter must not move, the other two still do).

Shapes: the headline's class, an enlargement (long runs of zero and of equal weights), two whose fractions are exactly 0 and 1/2, and a
picture in a rectangle of the canvas; chunk heights 4, 13, 52; 2, 3 and 4 layers; the three absorbed matrices mixed across layers; the
opacity sets of the carry test; random planes, all-0 planes (every tap the zero operand) and all-255 planes (the largest denormal).  The
identity itself runs on the device for every byte in every tap position over a weight grid, beside the sibling kernels' binary16 form.
Fixed seeds; nothing is skipped."""
import ctypes as C

import numpy as np
import pytest

import gpuutil as G
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv

pytestmark = pytest.mark.gpu

STREAM = "tick_bgra_stream"
F32, CARRY, OPAQUE = "stream_f32tap_launches", "stream_carry_launches", "stream_opaque_launches"
GEOMETRIES = [
    # canvas, source, rectangle of the picture on the canvas (None: the whole canvas)
    ((321, 70), (480, 104), None),                 # the headline's class
    ((321, 70), (160, 36), None),                  # enlarged: long runs of zero and equal weights
    ((320, 72), (160, 36), None),                  # 2 : 1 up: fractions of exactly 1/4 and 3/4
    ((320, 72), (320, 72), None),                  # 1 : 1: luma fractions exactly 0, chroma 1/4 and 3/4
    ((321, 70), (320, 90), (40, 5, 200, 60)),      # rows and columns outside the picture
]
OPACITIES = [(1.0, 0.75, 0.5, 0.25), (1.0, 0.0, 1.0, 0.3), (1.0, 1.0, 0.0, 0.6)]
CHUNK_ROWS = [4, 13, 52]
ABSORBED = [0, 1, 3]
CONTENT = ["random", "zeros", "full"]


def _cleared(cw, ch):
    exp = util.alloc_image("bgra", cw, ch)
    assert O.run_kernel("img_clear_bgra", exp) == 0
    return exp


def _source(fmt, sw, sh, seed, content):
    src = util.alloc_image(fmt, sw, sh, seed=seed)
    if content != "random":
        for plane in (src if isinstance(src, (list, tuple)) else [src]):
            np.asarray(plane)[...] = 0 if content == "zeros" else 255
    return src


def _layers(ctx, exp, canvas, src_size, ops, cscs, seed, rect, content):
    (cw, ch), (sw, sh) = canvas, src_size
    layers = []
    for i, (op, csc) in enumerate(zip(ops, cscs)):
        u = util.make_uniforms((cw, ch), in_size=(sw, sh), opacity=op, **({"rect": rect} if rect else {}))
        # (one layer of a non-random tick keeps random bytes: the blend must still see two different pictures)
        src = _source("nv12", sw, sh, seed + 7 * i, content if i != 1 else "random")
        assert O.run_kernel("img_nv12_bgra", exp, src, u, csc=csc, threads=8) == 0
        layers.append((sv.defaultComputeKernelFromString("img_nv12_bgra"), G.to_gpu(ctx, "nv12", sw, sh, src), u, csc))
    return layers


def _both_routes(ctx, switch, canvas, src_size, ops, cscs, rows, seed, rect=None, content="random"):
    """a batch through the f32-tap kernels and, with CHV_STREAM_F32TAPS=0, through the chroma-carry kernels they replace (carry on for both)"""
    cw, ch = canvas
    switch("CHV_BGRA_PATH", "stream")
    switch("CHV_STREAM_ROWS", str(rows))
    switch("CHV_STREAM_CARRY", "1")
    exp = _cleared(cw, ch)
    layers = _layers(ctx, exp, canvas, src_size, ops, cscs, seed, rect, content)
    for enabled in ("1", "0"):
        switch("CHV_STREAM_F32TAPS", enabled)
        what = f"CHV_STREAM_F32TAPS={enabled}, chunks of {rows} rows, {content}"
        gd = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=seed + 90))
        f0, c0, o0 = cv.get_counter(F32), cv.get_counter(CARRY), cv.get_counter(OPAQUE)
        h, name, keep = G.make_batch(ctx, [(gd, True, layers)])
        assert name == STREAM, f"dispatched to {name}"
        G.run_batch(ctx, h)
        G.destroy_batch(h)
        assert (cv.get_counter(F32) > f0) == (enabled == "1"), (what, "f32-tap counter", f0, cv.get_counter(F32))
        assert cv.get_counter(CARRY) > c0 and cv.get_counter(OPAQUE) > o0, (what, "carry / opaque counters")
        G.assert_same(G.from_gpu(ctx, gd, "bgra", cw, ch), exp, what)


@pytest.mark.parametrize("rows", CHUNK_ROWS)
@pytest.mark.parametrize("geom", range(len(GEOMETRIES)))
def test_f32_taps_match_oracle_and_the_carry_kernels(ctx, switch, geom, rows):
    canvas, src_size, rect = GEOMETRIES[geom]
    i = geom * len(CHUNK_ROWS) + CHUNK_ROWS.index(rows)
    nl = 2 + (i + geom) % 3                               # (every shape sees 2, 3 and 4 layers over its three chunk heights)
    cscs = [ABSORBED[(i + l) % 3] for l in range(nl)]
    _both_routes(ctx, switch, canvas, src_size, OPACITIES[(i // 3) % 3][:nl], cscs, rows, seed=9800 + 13 * i, rect=rect)


@pytest.mark.parametrize("content", ["zeros", "full"])
@pytest.mark.parametrize("geom", range(len(GEOMETRIES)))
def test_the_smallest_and_the_largest_taps(ctx, switch, geom, content):
    canvas, src_size, rect = GEOMETRIES[geom]
    nl = 2 + geom % 3
    _both_routes(ctx, switch, canvas, src_size, OPACITIES[geom % 3][:nl], [ABSORBED[(geom + l) % 3] for l in range(nl)], 13, seed=9900 + geom, rect=rect,
                 content=content)


@pytest.mark.parametrize("ops", range(len(OPACITIES)))
@pytest.mark.parametrize("nl", [2, 3, 4])
def test_every_layer_count_and_opacity_set_on_the_headline_shape(ctx, switch, nl, ops):
    _both_routes(ctx, switch, (321, 70), (480, 104), OPACITIES[ops][:nl], [ABSORBED[(ops + l) % 3] for l in range(nl)], 13, seed=9950 + 10 * nl + ops)


def test_the_switch_off_and_carry_off_take_neither(ctx, switch):
    """CHV_STREAM_CARRY=0 keeps tick_bgra_stream_ob whatever CHV_STREAM_F32TAPS says"""
    switch("CHV_BGRA_PATH", "stream")
    switch("CHV_STREAM_ROWS", "13")
    switch("CHV_STREAM_CARRY", "0")
    switch("CHV_STREAM_F32TAPS", "1")
    cw, ch = 321, 70
    exp = _cleared(cw, ch)
    layers = _layers(ctx, exp, (cw, ch), (480, 104), OPACITIES[0], [0, 1, 3, 0], 9990, None, "random")
    gd = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=9991))
    f0, c0, o0 = cv.get_counter(F32), cv.get_counter(CARRY), cv.get_counter(OPAQUE)
    h, name, keep = G.make_batch(ctx, [(gd, True, layers)])
    G.run_batch(ctx, h)
    G.destroy_batch(h)
    assert cv.get_counter(F32) == f0 and cv.get_counter(CARRY) == c0 and cv.get_counter(OPAQUE) > o0
    G.assert_same(G.from_gpu(ctx, gd, "bgra", cw, ch), exp, "carry off")


def test_the_identity_on_the_device_for_every_byte(ctx):
    """reference chain on converted floats == tap_h / cs_mix_h == cs_mix_d + fma(S, 2^22, m), as bits: every byte in every tap position with
    the others at 0 and 255, fractions {0, 2^-24, 2^-23, 1/4, 1/3, 1/2, 1 - 2^-24} squared (what lin_axis hands the kernels: [0, 1)), the nine
    conversion constants of the absorbed matrices in turn"""
    lib = cv.load()
    fn = lib.chv_selftest_f32_taps
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 5 + [C.c_int]
    grid = np.array([0.0, 2.0 ** -24, 2.0 ** -23, 0.25, 1.0 / 3.0, 0.5, 1.0 - 2.0 ** -24], dtype=np.float32)
    consts = np.array([10041594.0, 13672062.0, 9933686.0, 8659076.0, 15468090.0, 11137308.0, 8400986.0, -15564928.0, -9977984.0], dtype=np.float32)
    a, b, pos, oth, val = np.meshgrid(np.arange(grid.size), np.arange(grid.size), np.arange(4), np.array([0, 255]), np.arange(256), indexing="ij")
    n = a.size
    taps = np.repeat(oth.reshape(-1, 1), 4, axis=1).astype(np.uint32)
    taps[np.arange(n), pos.reshape(-1)] = val.reshape(-1)
    xa, ya = np.ascontiguousarray(grid[a.reshape(-1)]), np.ascontiguousarray(grid[b.reshape(-1)])
    m = np.ascontiguousarray(consts[np.arange(n) % 9])
    taps = np.ascontiguousarray(taps)
    out = np.zeros(3 * n, dtype=np.uint32)
    assert fn(xa.ctypes.data, ya.ctypes.data, taps.ctypes.data, m.ctypes.data, out.ctypes.data, n) == 0
    ref, mixh, dn = out[0::3], out[1::3], out[2::3]
    assert np.any(ref != ref[0]), "the self-test wrote nothing"
    # the reference chain against a float64 model of it where that is exact: one nonzero weight (fractions 0) — the sample is the byte
    exact = (a.reshape(-1) == 0) & (b.reshape(-1) == 0)
    want = (taps[exact, 0].astype(np.float32) + m[exact]).view(np.uint32)
    assert np.array_equal(ref[exact], want)
    bad = np.nonzero(mixh != ref)[0]
    assert bad.size == 0, f"cs_mix_h differs at {bad[:5]}"
    bad = np.nonzero(dn != ref)[0]
    assert bad.size == 0, f"cs_mix_d differs at {bad[:5]}: xa {xa[bad[:5]]} ya {ya[bad[:5]]} taps {taps[bad[:5]]} {[hex(v) for v in dn[bad[:5]]]} vs {[hex(v) for v in ref[bad[:5]]]}"
