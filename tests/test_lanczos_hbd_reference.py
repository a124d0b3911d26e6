"""The reference of chv_scale_lanczos_hbd_to_420's tests (tests/hbd_formats.py), pinned on the CPU:

  1. with scale 1 on 8-bit data the restated chain IS the oracle's (O.lanczos_bgra), byte for byte, over every tap class and both routes;
  2. the ignored bits of both formats (p010: low six, y420p10: high six) do not change it;
  3. it satisfies the independent float64 statement of tests/lanczos_f64.py: value = resample(codes) / 4, bound = delta * (1023 / 255) / 4
     (samples reach 1023 instead of 255; the final scaling is exact) — within the module's own cap on undecided samples — and the statement
     catches three wrong ones: scaling before the chain with a rounding, >> 2 truncation, word >> 6 taken for y420p10."""
import numpy as np
import pytest

import decoder_formats as D
import hbd_formats as H
import lanczos_f64 as F
import util

# (iw, ih, ow, oh): tap classes 6, 8, 12, 16, 22 and the tile route's 24, 30 and 40 taps; enlargements; odd sizes; one sample on an axis
CHAIN_SHAPES = [(2, 2, 2, 2), (2, 2, 4, 4), (1, 1, 2, 2), (1, 9, 1, 5), (34, 18, 34, 18), (20, 10, 66, 34), (40, 24, 30, 18), (66, 34, 40, 22),
                (96, 48, 40, 20), (33, 17, 21, 11), (130, 40, 40, 12), (700, 14, 200, 4), (64, 36, 17, 9), (96, 48, 20, 10), (40, 24, 6, 4)]
# the float64 table: the named shapes of tests/test_scale_lanczos_hbd_gpu.py in which no logical image passes through the identity on both axes
# (there a quarter of all codes are exact ties, which no bound decides; the first-principles GPU check covers those without a tolerance)
F64_SHAPES = [(66, 34, 40, 22), (20, 10, 66, 34), (38, 18, 21, 11), (33, 17, 21, 11), (200, 12, 150, 8), (130, 40, 40, 12), (96, 48, 20, 10),
              (40, 24, 6, 4)]


def test_with_scale_one_on_bytes_the_chain_is_the_oracles():
    classes = set()
    for iw, ih, ow, oh in CHAIN_SHAPES:
        img = util.splitmix_bytes(iw * 131 + oh, iw * ih).reshape(ih, iw)
        got = H.resize(img, ow, oh, scale=1.0)
        assert np.array_equal(got, D.resize(img, ow, oh)), (iw, ih, ow, oh)
        t = max(D.taps(iw, ow), D.taps(ih, oh))
        classes.add(6 if t <= 6 else 8 if t <= 8 else 12 if t <= 12 else 16 if t <= 16 else 22 if t <= 22 else "tile")
    assert classes == {6, 8, 12, 16, 22, "tile"}, classes


def test_the_final_scaling_rounds_once_ties_to_even_and_saturates():
    codes = np.arange(1024, dtype=np.uint16).reshape(32, 32)
    got = H.resize(codes, 32, 32)
    assert np.array_equal(got, np.minimum(np.rint(codes / 4.0), 255).astype(np.uint8))
    assert got.reshape(-1)[[2, 6, 10, 1022, 1023]].tolist() == [0, 2, 2, 255, 255]


@pytest.mark.parametrize("sfmt", H.FORMATS)
def test_the_ignored_bits_do_not_change_the_reference(sfmt):
    iw, ih, ow, oh = 38, 18, 21, 11
    codes = H.random_codes(iw, ih, 5)
    clean, a, b = (H.pack(sfmt, *codes, seed=s) for s in (None, 1, 2))
    assert any(not np.array_equal(x, y) for x, y in zip(a, b)) and any(not np.array_equal(x, y) for x, y in zip(a, clean))
    for x, y in zip(H.codes_of(sfmt, a), codes):
        assert np.array_equal(x, y)
    for dfmt in H.TARGETS:
        want = H.reference(sfmt, dfmt, clean, ow, oh)
        for planes in (a, b):
            for g, e in zip(H.reference(sfmt, dfmt, planes, ow, oh), want):
                assert np.array_equal(g, e)
        for g, e in zip(H.case(sfmt, dfmt, iw, ih, ow, oh, 5)[1], want):
            assert np.array_equal(g, e)


# ---- the float64 statement -----------------------------------------------------------------------------------------------------------------
def interval(codes, ow, oh):
    """(lo, hi, undecided) of one logical image of 10-bit codes"""
    ih, iw = codes.shape
    v = F.resample(codes, ow, oh) / 4.0
    d = F.delta(iw, ih, ow, oh) * (1023.0 / 255.0) / 4.0
    lo, hi = F.sat_rte(v - d), F.sat_rte(v + d)
    assert ((hi - lo) >= 0).all() and ((hi - lo) <= 1).all()
    return lo, hi


def hold(shape, stored, shares=None, what="reference"):
    """stored(codes, ow, oh) of every logical image of the shape's seeded picture against its interval"""
    iw, ih, ow, oh = shape
    sizes = H.logical_sizes(ow, oh)
    for name, codes, (w, h) in zip("Y Cb Cr".split(), H.random_codes(iw, ih, iw * 7 + oh), (sizes[0], sizes[1], sizes[1])):
        lo, hi = interval(codes, w, h)
        if shares is not None:
            shares.add(lo != hi, lo.size, "%s %dx%d -> %dx%d plane %s" % ((what,) + shape + (name,)))
        F.assert_within(lo, hi, stored(codes, w, h), "%s %dx%d -> %dx%d plane %s" % ((what,) + shape + (name,)))


def test_the_reference_satisfies_the_float64_statement_inside_the_cap():
    shares = F.Shares(F.PLAIN_CAP)
    for shape in F64_SHAPES:
        hold(shape, H.resize, shares)
    shares.assert_pool("the pooled small planes of the table")


def test_the_statement_catches_wrong_ones():
    wrong = {
        "scaled before the chain, with a rounding": lambda c, w, h: H.resize(np.rint(c / 4.0).astype(np.uint16), w, h, scale=1.0),
        "scaled before the chain, >> 2": lambda c, w, h: H.resize(c >> 2, w, h, scale=1.0),
        # y420p10 words with garbage above the code, read as p010 reads its words
        "word >> 6 taken for y420p10": lambda c, w, h: H.resize(H.pack("y420p10", c, c, c, seed=3)[0] >> 6, w, h),
    }
    # A wrong statement moves a few per cent of the samples across a rounding boundary (an input error of up to half an 8-bit code, filtered),
    # so a picture of some hundred samples shows it and one of 6 x 4 need not: every shape whose luma is not pooled (F.POOL_BELOW) must catch it.
    large = [s for s in F64_SHAPES if s[2] * s[3] >= F.POOL_BELOW]
    assert len(large) >= 4
    for what, stored in wrong.items():
        for shape in large:
            with pytest.raises(AssertionError):
                hold(shape, stored, what=what)
