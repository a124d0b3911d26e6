"""chv_scale_lanczos_to_420 / chv_scale_lanczos_to_420_ladder against the float64 statement of tests/lanczos_f64.py (DESIGN.md sections 4.4 and
4.4.9) — directly: nothing here comes from oracle/ref_kernels.c.  The entries store the resample of every logical image, so they are held to
the PLAIN check, sample by sample, with every image's own matrices: |code - v| <= 0.5 + delta, an F.Plane per logical image.  The cap
(F.PLAIN_CAP: at most 2 % of a plane undecided, small planes pooled) is a condition on the inputs, counted from the statement alone — also on the
CPU, without a device (test_the_statement_alone_stays_inside_the_cap).

The GPU cases are a table run by ONE test; the CPU test counts the cap over the same table.  The shapes and content kinds are those of tests/test_gpu_lanczos_f64.py for the five source formats into both targets.  Two kinds of cell are
not cases: a packed 4:2:2 picture has an even width, and a shape in which the 160 KB rule of chv_scale_lanczos refuses a logical image is
refused by the entry (600x64 -> 50x8 from a 4:4:4 source: its chroma is reduced 24:1 by 16:1)."""
import functools

import numpy as np
import pytest

import decoder_formats as D
import gpuutil as G
import lanczos_f64 as F
import util
from test_gpu_lanczos_f64 import IDENTITY, KINDS, LADDER_RUNGS, LADDER_SRC, SHAPES, blocks, fill, logical, plain, seed_of

from swiftvideo_amd import compute as sv

CELLS = [(s, d) for s in D.FORMATS for d in D.TARGETS]


def is_case(sfmt, dfmt, shape):
    return not (sfmt in D.PACKED and shape[0] % 2) and not D.refused(sfmt, dfmt, *shape)


CASES = [pytest.param(s, d, shape, id="%s-to-%s-%dx%d-%dx%d" % ((s, d) + shape)) for shape in SHAPES for s, d in CELLS if is_case(s, d, shape)]
assert len(CASES) >= 8 * len(SHAPES)


@functools.lru_cache(maxsize=None)
def source(fmt, iw, ih, seed, kind="random"):
    """(Y, Cb, Cr) of a picture of format `fmt` (the chroma sizes are the format's): seeded bytes, or flat 8 x 8 blocks of the range limits"""
    (yw, yh), (cw, ch) = D.logical_sizes(fmt, iw, ih)
    if kind == "random":
        planes = tuple(util.splitmix_bytes(seed * 16 + k, r * c).reshape(r, c).copy() for k, (r, c) in enumerate([(yh, yw), (ch, cw), (ch, cw)]))
    else:
        rng = np.random.default_rng(seed)
        planes = (blocks(rng, yh, yw, (0, 255, 16, 235)), blocks(rng, ch, cw, (0, 255, 16, 240)), blocks(rng, ch, cw, (0, 255, 16, 240)))
    for a in planes:
        a.setflags(write=False)
    return planes


def size_class(fmt):
    """formats whose logical images have the same sizes share their references"""
    return "y422p" if fmt in D.PACKED else fmt


@functools.lru_cache(maxsize=None)
def ref(cls, iw, ih, ow, oh, seed, kind="random"):
    y, cb, cr = source(cls, iw, ih, seed, kind)
    (tw, th), (cw, ch) = D.logical_sizes("nv12", ow, oh)
    return F.Plane(y, tw, th), F.Plane(cb, cw, ch), F.Plane(cr, cw, ch)


def case(ctx, sfmt, dfmt, shape, kind, shares, sources=None):
    iw, ih, ow, oh = shape
    seed = seed_of(*shape)
    cls = size_class(sfmt)
    got = None
    if ctx is not None:
        src = source(cls, iw, ih, seed, kind)
        gs = sources.place(sfmt, iw, ih, D.pack(sfmt, *src), "vector")
        gd = fill(ctx, dfmt, ow, oh, seed + 7)
        sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420(c, gd, gs))
        got = logical(dfmt, G.from_gpu(ctx, gd, dfmt, ow, oh))
        if shape == IDENTITY:
            assert np.array_equal(got[0], src[0]), "equal sizes: Y itself"
    plain(f"to_420 {sfmt}->{dfmt} {kind}", shape, ["Y", "Cb", "Cr"], ref(cls, iw, ih, ow, oh, seed, kind), got, shares, "%dx%d -> %dx%d" % shape)


def test_the_statement_alone_stays_inside_the_cap():
    """CPU: the undecided share of every case's planes, counted from the float64 statement alone, against F.PLAIN_CAP — small planes pooled"""
    shares = F.Shares(F.PLAIN_CAP)
    for kind in KINDS:
        for p in CASES:
            sfmt, dfmt, shape = p.values
            if dfmt == "nv12":                  # (the planes of the two targets are the same logical images)
                case(None, sfmt, dfmt, shape, kind, shares)
    shares.assert_pool("the pooled small planes of every case")


def check_single(ctx, sfmt, dfmt, shape, kind):
    shares, sources = F.Shares(F.PLAIN_CAP), D.Sources(ctx)
    case(ctx, sfmt, dfmt, shape, kind, shares, sources)
    sources.unchanged()


def check_ladder(ctx, sfmt, dfmt):
    """one source size, four rungs — strip rungs of both variants, a tile rung and an enlargement: a rung that read another rung's table would
    show here without the single call as a go-between"""
    iw, ih = LADDER_SRC
    shares, cls = F.Shares(F.PLAIN_CAP), size_class(sfmt)
    srcs = [source(cls, iw, ih, 900 + i) for i in range(2)]
    gs = [D.to_gpu(ctx, sfmt, iw, ih, D.pack(sfmt, *s)) for s in srcs]
    rungs = [[fill(ctx, dfmt, w, h, 30 + 4 * r + i) for i in range(2)] for r, (w, h) in enumerate(LADDER_RUNGS)]
    sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420Ladder(c, rungs, gs))
    for r, (w, h) in enumerate(LADDER_RUNGS):
        for i in range(2):
            got = logical(dfmt, G.from_gpu(ctx, rungs[r][i], dfmt, w, h))
            plain(f"to_420 ladder {sfmt}->{dfmt}", (iw, ih, w, h), ["Y", "Cb", "Cr"], ref(cls, iw, ih, w, h, 900 + i), got, shares, f"rung {r} of source {i}")
    shares.assert_pool(f"ladder {sfmt} -> {dfmt}")


@pytest.mark.gpu
def test_chv_scale_lanczos_to_420_against_the_float64_statement(ctx):
    """every case of CASES with both content kinds, then one ladder per source format: a table run by one test (two seconds together), every
    case whether or not an earlier one failed, each failed case reported by its name; anything but a failed assertion ends the test at once"""
    table = [("%s-%s" % (p.id, kind), check_single, p.values + (kind,)) for kind in KINDS for p in CASES]
    table += [("ladder-%s-to-%s" % (s, D.TARGETS[i % 2]), check_ladder, (s, D.TARGETS[i % 2])) for i, s in enumerate(D.FORMATS)]
    assert len(table) == 2 * len(CASES) + 5
    failed = []
    for name, check, args in table:
        try:
            check(ctx, *args)
        except AssertionError as e:
            failed.append(f"{name}: {str(e)[:600]}")
    assert not failed, "%d case(s) failed:\n%s" % (len(failed), "\n".join(failed[:20]))
