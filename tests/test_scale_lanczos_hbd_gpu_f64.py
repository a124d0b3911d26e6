"""chv_scale_lanczos_hbd_to_420 / chv_scale_lanczos_hbd_to_420_ladder against the float64 statement of tests/lanczos_f64.py (DESIGN.md sections
4.4 and 4.4.10) — directly: nothing here comes from the restated chain of tests/hbd_formats.py or from oracle/ref_kernels.c.  Per logical image
of 10-bit codes the value is resample(codes, ow, oh) / 4 and the bound delta(iw, ih, ow, oh) * (1023 / 255) / 4: samples reach 1023 instead of
255, and the final scaling is exact.  A stored byte must lie in [sat_rte(v - d), sat_rte(v + d)]; the module's caps (F.PLAIN_CAP: at most 2 %
of a plane undecided, planes below 400 samples pooled) are conditions on the inputs, asserted for the same seeds on the CPU by
tests/test_lanczos_hbd_reference.py.  The table is that test's: the named shapes in which no logical image passes through the identity on both
axes (there a quarter of all codes are exact ties; tests/test_scale_lanczos_hbd_gpu.py checks those geometries from first principles)."""
import pytest

import gpuutil as G
import hbd_formats as H
import lanczos_f64 as F
import util
from swiftvideo_amd import compute as sv
from test_gpu_lanczos_f64 import logical
from test_lanczos_hbd_reference import F64_SHAPES, interval

CELLS = [(s, d) for s in H.FORMATS for d in H.TARGETS]


def hold(shape, codes, got, shares, what):
    sizes = H.logical_sizes(shape[2], shape[3])
    for name, c, g, (w, h) in zip("Y Cb Cr".split(), codes, got, (sizes[0], sizes[1], sizes[1])):
        lo, hi = interval(c, w, h)
        shares.add(lo != hi, lo.size, f"{what} plane {name}")
        F.assert_within(lo, hi, g, f"{what} plane {name}")


def check_single(ctx, sfmt, dfmt, shape):
    iw, ih, ow, oh = shape
    seed = iw * 7 + oh
    codes = H.random_codes(iw, ih, seed)
    sources, shares = H.Sources(ctx), F.Shares(F.PLAIN_CAP)
    gs = sources.place(sfmt, iw, ih, H.pack(sfmt, *codes, seed=seed), "vector")
    gd = G.to_gpu(ctx, dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=seed + 7))
    sv.usingContext(ctx, lambda c: sv.scaleLanczosHbdTo420(c, gd, gs))
    hold(shape, codes, logical(dfmt, G.from_gpu(ctx, gd, dfmt, ow, oh)), shares, "hbd %s->%s %dx%d -> %dx%d" % ((sfmt, dfmt) + shape))
    sources.unchanged()


def check_ladder(ctx, sfmt, dfmt):
    """one source size, four rungs — strip rungs of both variants, a tile rung and an enlargement: a rung that read another rung's table would
    show here without the single call as a go-between"""
    iw, ih = 96, 48
    sizes = [(64, 32), (30, 16), (20, 10), (130, 66)]
    assert [H.tap_class(sfmt, dfmt, iw, ih, w, h)[0] for w, h in sizes] == [10, 20, 30, 6]
    shares = F.Shares(F.PLAIN_CAP)
    codes = [H.random_codes(iw, ih, 900 + i) for i in range(2)]
    gs = [H.to_gpu(ctx, sfmt, iw, ih, H.pack(sfmt, *c, seed=i)) for i, c in enumerate(codes)]
    rungs = [[G.to_gpu(ctx, dfmt, w, h, util.alloc_image(dfmt, w, h, seed=30 + 4 * r + i)) for i in range(2)] for r, (w, h) in enumerate(sizes)]
    sv.usingContext(ctx, lambda c: sv.scaleLanczosHbdTo420Ladder(c, rungs, gs))
    for r, (w, h) in enumerate(sizes):
        for i in range(2):
            hold((iw, ih, w, h), codes[i], logical(dfmt, G.from_gpu(ctx, rungs[r][i], dfmt, w, h)), shares, f"hbd ladder {sfmt}->{dfmt} rung {r} of source {i}")
    shares.assert_pool(f"ladder {sfmt} -> {dfmt}")


@pytest.mark.gpu
def test_chv_scale_lanczos_hbd_to_420_against_the_float64_statement(ctx):
    """every shape of the table for both sources and both targets, then one ladder per cell: a table run by one test, every case whether or not
    an earlier one failed, each failed case reported by its name; anything but a failed assertion ends the test at once"""
    table = [("%s-to-%s-%dx%d-%dx%d" % ((s, d) + shape), check_single, (s, d, shape)) for shape in F64_SHAPES for s, d in CELLS]
    table += [("ladder-%s-to-%s" % (s, d), check_ladder, (s, d)) for s, d in CELLS]
    assert len(table) == 4 * len(F64_SHAPES) + 4
    failed = []
    for name, check, args in table:
        try:
            check(ctx, *args)
        except AssertionError as e:
            failed.append(f"{name}: {str(e)[:600]}")
    assert not failed, "%d case(s) failed:\n%s" % (len(failed), "\n".join(failed[:20]))
