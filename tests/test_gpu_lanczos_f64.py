"""Every Lanczos-3 entry of the C ABI against the float64 statement of tests/lanczos_f64.py — directly: nothing here
comes from oracle/ref_kernels.c, whose table builder was written from the same formula as the product's.

Entries that store the resample are held to the PLAIN check, sample by sample, with every plane's own matrices: |code - v| <= 0.5 + delta.
Entries that put integer arithmetic behind it (sections 4.2, 4.4.2, 4.5) are held to the INTERVAL check: a stored byte lies between the
matrix's values at the corners of [lo, hi] that its signs name — equality wherever the samples are decided.  The caps of lanczos_f64 bound what
the intervals may hide and are asserted on every case, counted from the statement alone.  Every target is pre-filled with seeded bytes and
whole planes are compared; no sample is left out.

Each test prints one `f64:` line per compared plane (pytest -s): the largest |code - v| - 0.5 beside the largest delta (plain check), and the
undecided share."""
import functools

import numpy as np
import pytest

import gpuutil as G
import lanczos_f64 as F
import util
from swiftvideo_amd import compute as sv
from test_gpu_lanczos_from_yuv import source_to_gpu as picture_to_gpu          # (describes the planes of a 1-wide or 1-high picture by hand)

pytestmark = pytest.mark.gpu

FORMATS = ["nv12", "y420p"]
ORDERS = ["bgra", "rgba"]
CROSS = [("nv12", "y420p"), ("y420p", "nv12")]
KINDS = ["random", "blocks"]
SHAPES = [(36, 20, 24, 14),          # 10 and 6 taps, the short strip template
          (440, 220, 200, 100),      # 14 and 8 taps
          (700, 140, 200, 40),       # 22 taps, the strip route's edge
          (64, 36, 17, 9),           # 24 taps, the tile route
          (600, 64, 50, 8),          # 72 taps, small tiles, the slow tap loop
          (33, 17, 20, 10),          # odd source; tap counts differ between axes and between planes
          (100, 50, 333, 171),       # enlargement, several output rows per source row
          (1100, 40, 550, 20),       # several strips, the last one partial
          (2, 2, 7, 5), (1, 1, 5, 3),          # 1 x 1 chroma, all clamps
          (5, 3, 1, 1),              # degenerate target
          (16, 16, 16, 16)]          # identity; must be exact
IDS = ["%dx%d-%dx%d" % s for s in SHAPES]
IDENTITY = (16, 16, 16, 16)
# one source size, four rungs: a strip rung of at most 12 taps, one of at most 22, a tile rung (24 taps) and an enlargement
LADDER_SRC, LADDER_RUNGS = (288, 144), [(192, 96), (82, 41), (72, 36), (400, 200)]


def blocks(rng, h, w, values):
    """flat 8 x 8 blocks of seeded picks from `values`"""
    picks = rng.choice(np.array(values, dtype=np.uint8), size=((h + 7) // 8, (w + 7) // 8))
    return np.ascontiguousarray(np.kron(picks, np.ones((8, 8), dtype=np.uint8))[:h, :w])


def chroma_size(w, h):
    return max(1, w // 2), max(1, h // 2)


def seed_of(iw, ih, ow, oh):
    return iw * 7 + oh


# ---- sources and their float64 references: computed once per shape, shared, left unchanged ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def source4(iw, ih, seed, kind="random"):
    """one (ih, iw, 4) plane: seeded bytes, or flat 8 x 8 blocks of {0, 255, 16, 235} per component, whose ringing reaches the saturation"""
    if kind == "random":
        a = util.splitmix_bytes(seed * 16 + 9, ih * iw * 4).reshape(ih, iw, 4).copy()
    else:
        rng = np.random.default_rng(seed)
        a = np.ascontiguousarray(np.stack([blocks(rng, ih, iw, (0, 255, 16, 235)) for _ in range(4)], axis=-1))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def source420(iw, ih, seed, kind="random"):
    """(Y, Cb, Cr): seeded bytes, or flat 8 x 8 blocks of the range limits"""
    cw, ch = chroma_size(iw, ih)
    if kind == "random":
        planes = tuple(util.splitmix_bytes(seed * 16 + k, r * c).reshape(r, c).copy() for k, (r, c) in enumerate([(ih, iw), (ch, cw), (ch, cw)]))
    else:
        rng = np.random.default_rng(seed)
        planes = (blocks(rng, ih, iw, (0, 255, 16, 235)), blocks(rng, ch, cw, (0, 255, 16, 240)), blocks(rng, ch, cw, (0, 255, 16, 240)))
    for a in planes:
        a.setflags(write=False)
    return planes


def packed(fmt, y, cb, cr):
    return [y.copy(), np.ascontiguousarray(np.stack([cb, cr], axis=-1))] if fmt == "nv12" else [y.copy(), cb.copy(), cr.copy()]


def logical(fmt, planes):
    if fmt == "nv12":
        return np.asarray(planes[0]), np.asarray(planes[1])[..., 0], np.asarray(planes[1])[..., 1]
    return tuple(np.asarray(p) for p in planes)


@functools.lru_cache(maxsize=None)
def ref4(iw, ih, ow, oh, seed, kind="random"):
    return F.Plane(source4(iw, ih, seed, kind), ow, oh)


@functools.lru_cache(maxsize=None)
def ref420(iw, ih, ow, oh, seed, kind="random"):
    """Y, Cb and Cr each resampled as a picture of its own: luma to ow x oh, chroma to the target's chroma size — each plane's own matrices"""
    y, cb, cr = source420(iw, ih, seed, kind)
    cw, ch = chroma_size(ow, oh)
    return F.Plane(y, ow, oh), F.Plane(cb, cw, ch), F.Plane(cr, cw, ch)


@functools.lru_cache(maxsize=None)
def ref_from(iw, ih, ow, oh, seed):
    """Y, Cb and Cr each resampled to ow x oh (section 4.4.6)"""
    return tuple(F.Plane(p, ow, oh) for p in source420(iw, ih, seed))


def fill(ctx, fmt, w, h, seed):
    """a target pre-filled with seeded bytes"""
    planes = util.alloc_image(fmt, w, h, seed=seed)
    return G.to_gpu(ctx, fmt, w, h, planes) if fmt in ORDERS else picture_to_gpu(ctx, fmt, w, h, planes)


def line(entry, shape, plane, share, worst=None, d=None):
    """plain check: the largest |code - v| - 0.5 beside the largest delta (how loose the derived bound is; no tolerance); interval check: the
    share of bytes the interval leaves open — every other byte was compared for equality"""
    figures = "interval" if worst is None else "worst %+.3e  delta %.3e" % (worst, d)
    print("f64: %-28s %-18s %-6s %s  undecided %.3f %%" % (entry, "%dx%d-%dx%d" % tuple(shape), plane, figures, 100 * share))


# ---- the two checks --------------------------------------------------------------------------------------------------------------------------
def plain(entry, shape, names, refs, got, shares, what):
    """the plain check of every plane, its cap, and one report line per plane; `got` None: only the cap is counted (the pooled count below)"""
    for name, ref, g in zip(names, refs, got or [None] * len(refs)):
        share = shares.add(ref.undecided, ref.v.shape[0] * ref.v.shape[1], f"{entry} {what}, plane {name}")
        if g is not None:
            F.assert_plain(ref, g, f"{entry} {what}, plane {name}")
            line(entry, shape, name, share, *ref.looseness(g))
            if tuple(shape) == IDENTITY:
                assert not ref.undecided.any()


def within(entry, shape, names, intervals, got, samples, shares, what, colour=None):
    for name, (lo, hi), g in zip(names, intervals, got or [None] * len(intervals)):
        counted = (lo != hi) if colour is None else (lo != hi)[..., colour]
        share = shares.add(counted, samples, f"{entry} {what}, plane {name}")
        if g is not None:
            F.assert_within(lo, hi, g, f"{entry} {what}, plane {name}")
            line(entry, shape, name, share)


# ---- 1. chv_scale_lanczos: one 4-component plane, NV12, y420p -------------------------------------------------------------------------------------
def bgra_case(ctx, shape, kind, shares):
    iw, ih, ow, oh = shape
    seed = seed_of(*shape)
    got = None
    if ctx is not None:
        gs = G.to_gpu(ctx, "bgra", iw, ih, [source4(iw, ih, seed, kind)])
        gd = fill(ctx, "bgra", ow, oh, seed + 7)
        sv.usingContext(ctx, lambda c: sv.scaleLanczos(c, gd, gs))
        got = G.from_gpu(ctx, gd, "bgra", ow, oh)
        if shape == IDENTITY:
            assert np.array_equal(got[0], source4(iw, ih, seed, kind)), "equal sizes: the plane itself"
    plain("scale_lanczos bgra " + kind, shape, ["BGRA"], [ref4(iw, ih, ow, oh, seed, kind)], got, shares, "%dx%d -> %dx%d" % shape)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_scale_lanczos_four_components(ctx, shape, kind):
    bgra_case(ctx, shape, kind, F.Shares(F.PLAIN_CAP))


def planar_case(ctx, shape, sfmt, dfmt, shares, kind="random"):
    """chv_scale_lanczos for a same-format pair, chv_scale_lanczos_420 for a cross pair: the logical planes, each with its own matrices"""
    iw, ih, ow, oh = shape
    seed = seed_of(*shape)
    entry = f"scale_lanczos {sfmt} {kind}" if sfmt == dfmt else f"420 {sfmt}->{dfmt}"
    got = None
    if ctx is not None:
        src = source420(iw, ih, seed, kind)
        gs = picture_to_gpu(ctx, sfmt, iw, ih, packed(sfmt, *src))
        gd = fill(ctx, dfmt, ow, oh, seed + 7)
        sv.usingContext(ctx, lambda c: (sv.scaleLanczos if sfmt == dfmt else sv.scaleLanczos420)(c, gd, gs))
        got = logical(dfmt, G.from_gpu(ctx, gd, dfmt, ow, oh))
        if shape == IDENTITY:
            assert all(np.array_equal(g, s) for g, s in zip(got, src)), "equal sizes: the planes themselves"
    plain(entry, shape, ["Y", "Cb", "Cr"], ref420(iw, ih, ow, oh, seed, kind), got, shares, "%dx%d -> %dx%d" % shape)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_scale_lanczos_420_pictures(ctx, shape, fmt, kind):
    planar_case(ctx, shape, fmt, fmt, F.Shares(F.PLAIN_CAP), kind)


# ---- 2. chv_scale_lanczos_420: both cross pairs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfmt,dfmt", CROSS, ids=["nv12-to-y420p", "y420p-to-nv12"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_scale_lanczos_420_cross_pairs(ctx, shape, sfmt, dfmt):
    planar_case(ctx, shape, sfmt, dfmt, F.Shares(F.PLAIN_CAP))


# ---- 3. chv_scale_lanczos_to_yuv ------------------------------------------------------------------------------------------------------------------
def to_yuv_csc(i, fmt, order):
    """the colourspaces spread over the cases"""
    return (i + FORMATS.index(fmt) + 2 * ORDERS.index(order)) % 4


def to_yuv_case(ctx, shape, fmt, order, csc, shares):
    iw, ih, ow, oh = shape
    seed = seed_of(*shape)
    ref = ref4(iw, ih, ow, oh, seed)
    got = None
    if ctx is not None:
        gs = G.to_gpu(ctx, order, iw, ih, [source4(iw, ih, seed)])
        gd = fill(ctx, fmt, ow, oh, seed + 7)
        sv.usingContext(ctx, lambda c: sv.scaleLanczosToYuv(c, gd, gs, colorspace=csc))
        got = logical(fmt, G.from_gpu(ctx, gd, fmt, ow, oh))
    intervals = F.to_yuv_interval(csc, order, ref)
    for (lo, hi), (w, h) in zip(intervals, [(ow, oh), chroma_size(ow, oh), chroma_size(ow, oh)]):
        assert lo.shape == (h, w)
    names = ["Y", "Cb", "Cr"]
    for k in range(3):
        within(f"to_yuv {order}->{fmt} csc{csc}", shape, names[k:k + 1], intervals[k:k + 1], None if got is None else got[k:k + 1],
               intervals[k][0].size, shares, "%dx%d -> %dx%d" % shape)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_scale_lanczos_to_yuv(ctx, i, fmt, order):
    to_yuv_case(ctx, SHAPES[i], fmt, order, to_yuv_csc(i, fmt, order), F.Shares(F.MATRIX_CAP))


# ---- 4. chv_scale_lanczos_from_yuv ----------------------------------------------------------------------------------------------------------------
def from_yuv_case(ctx, shape, sfmt, dfmt, csc, shares, seed=None, batch=None):
    iw, ih, ow, oh = shape
    seed = seed_of(*shape) if seed is None else seed
    got = None
    if ctx is not None:
        got = batch if batch is not None else None
        if got is None:
            gs = picture_to_gpu(ctx, sfmt, iw, ih, packed(sfmt, *source420(iw, ih, seed)))
            gd = fill(ctx, dfmt, ow, oh, seed + 7)
            sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuv(c, gd, gs, colorspace=csc))
            got = G.from_gpu(ctx, gd, dfmt, ow, oh)
        assert (got[0][..., 3] == 255).all(), "alpha is 255 exactly"
    interval = F.from_yuv_interval(csc, dfmt, *ref_from(iw, ih, ow, oh, seed))
    assert (interval[0][..., 3] == 255).all() and (interval[1][..., 3] == 255).all()
    within(f"from_yuv {sfmt}->{dfmt} csc{csc}", shape, [dfmt.upper()], [interval], got, ow * oh, shares, "%dx%d -> %dx%d" % shape,
           colour=slice(0, 3))          # (the share is of the colour bytes: the alpha bytes are always decided)


@pytest.mark.parametrize("dfmt", ORDERS)
@pytest.mark.parametrize("sfmt", FORMATS)
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_scale_lanczos_from_yuv(ctx, i, sfmt, dfmt):
    from_yuv_case(ctx, SHAPES[i], sfmt, dfmt, to_yuv_csc(i, sfmt, dfmt), F.Shares(F.MATRIX_CAP))


# ---- 5. ladders and a batch: a rung that reads another rung's table is caught here, without the single call as a go-between ----------------------------
def targets(ctx, fmt, n, seed):
    return [[fill(ctx, fmt, w, h, seed + 16 * r + i) for i in range(n)] for r, (w, h) in enumerate(LADDER_RUNGS)]


def ladder_planar_case(ctx, sfmt, dfmt, shares):
    n, (iw, ih) = 2, LADDER_SRC
    entry = "ladder " + sfmt if sfmt == dfmt else f"420_ladder {sfmt}->{dfmt}"
    rungs = None
    if ctx is not None:
        gs = [G.to_gpu(ctx, sfmt, iw, ih, packed(sfmt, *source420(iw, ih, 900 + i))) for i in range(n)]
        rungs = targets(ctx, dfmt, n, 3)
        sv.usingContext(ctx, lambda c: (sv.scaleLanczosLadder if sfmt == dfmt else sv.scaleLanczos420Ladder)(c, rungs, gs))
    for r, (ow, oh) in enumerate(LADDER_RUNGS):
        for i in range(n):
            got = None if rungs is None else logical(dfmt, G.from_gpu(ctx, rungs[r][i], dfmt, ow, oh))
            plain(entry, (iw, ih, ow, oh), ["Y", "Cb", "Cr"], ref420(iw, ih, ow, oh, 900 + i), got, shares, f"rung {r} ({ow}x{oh}) of source {i}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_ladder_of_420_pictures(ctx, fmt):
    ladder_planar_case(ctx, fmt, fmt, F.Shares(F.PLAIN_CAP))


@pytest.mark.parametrize("sfmt,dfmt", CROSS, ids=["nv12-to-y420p", "y420p-to-nv12"])
def test_ladder_between_the_packings(ctx, sfmt, dfmt):
    ladder_planar_case(ctx, sfmt, dfmt, F.Shares(F.PLAIN_CAP))


def ladder_to_yuv_case(ctx, fmt, order, csc, shares):
    n, (iw, ih) = 2, LADDER_SRC
    rungs = None
    if ctx is not None:
        gs = [G.to_gpu(ctx, order, iw, ih, [source4(iw, ih, 900 + i)]) for i in range(n)]
        rungs = targets(ctx, fmt, n, 5)
        sv.usingContext(ctx, lambda c: sv.scaleLanczosToYuvLadder(c, rungs, gs, colorspace=csc))
    for r, (ow, oh) in enumerate(LADDER_RUNGS):
        for i in range(n):
            got = None if rungs is None else logical(fmt, G.from_gpu(ctx, rungs[r][i], fmt, ow, oh))
            intervals = F.to_yuv_interval(csc, order, ref4(iw, ih, ow, oh, 900 + i))
            for k, name in enumerate(["Y", "Cb", "Cr"]):
                within(f"to_yuv_ladder {order}->{fmt} csc{csc}", (iw, ih, ow, oh), [name], intervals[k:k + 1], None if got is None else got[k:k + 1],
                       intervals[k][0].size, shares, f"rung {r} ({ow}x{oh}) of source {i}")


@pytest.mark.parametrize("fmt,order,csc", [("nv12", "bgra", 1), ("y420p", "rgba", 2)])
def test_ladder_into_420_pictures(ctx, fmt, order, csc):
    ladder_to_yuv_case(ctx, fmt, order, csc, F.Shares(F.MATRIX_CAP))


BATCH_SHAPE, BATCH_N = (146, 40, 73, 20), 3          # 12 luma taps; chroma 73 x 20 -> 73 x 20 is 1 : 1


def batch_from_yuv_case(ctx, sfmt, dfmt, csc, shares):
    iw, ih, ow, oh = BATCH_SHAPE
    gots = [None] * BATCH_N
    if ctx is not None:
        gs = [G.to_gpu(ctx, sfmt, iw, ih, packed(sfmt, *source420(iw, ih, 700 + i))) for i in range(BATCH_N)]
        gd = [fill(ctx, dfmt, ow, oh, 20 + i) for i in range(BATCH_N)]
        sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuvBatch(c, list(zip(gd, gs)), colorspace=csc))
        gots = [G.from_gpu(ctx, g, dfmt, ow, oh) for g in gd]
    for i in range(BATCH_N):
        from_yuv_case(ctx, BATCH_SHAPE, sfmt, dfmt, csc, shares, seed=700 + i, batch=gots[i])


@pytest.mark.parametrize("sfmt,dfmt,csc", [("nv12", "rgba", 3), ("y420p", "bgra", 0)])
def test_batch_of_three_from_yuv(ctx, sfmt, dfmt, csc):
    batch_from_yuv_case(ctx, sfmt, dfmt, csc, F.Shares(F.MATRIX_CAP))


# ---- 6. the pooled caps: every case above once more, counted from the statement alone ---------------------------------------------------------------
def test_the_small_planes_hold_the_caps_together():
    """(CPU work on the cached references) a plane of fewer than 400 samples is too small for a share of its own: all of them together are
    held to the same caps, one count for the resampled planes and one for the planes behind a matrix"""
    plain_shares, matrix_shares = F.Shares(F.PLAIN_CAP), F.Shares(F.MATRIX_CAP)
    for i, shape in enumerate(SHAPES):
        for kind in KINDS:
            bgra_case(None, shape, kind, plain_shares)
            for fmt in FORMATS:
                planar_case(None, shape, fmt, fmt, plain_shares, kind)
        for sfmt, dfmt in CROSS:
            planar_case(None, shape, sfmt, dfmt, plain_shares)
        for fmt in FORMATS:
            for order in ORDERS:
                to_yuv_case(None, shape, fmt, order, to_yuv_csc(i, fmt, order), matrix_shares)
                from_yuv_case(None, shape, fmt, order, to_yuv_csc(i, fmt, order), matrix_shares)
    assert plain_shares.pool_n > 1000 and matrix_shares.pool_n > 1000
    plain_shares.assert_pool("resampled planes below 400 samples")
    matrix_shares.assert_pool("planes behind a matrix, below 400 samples")
