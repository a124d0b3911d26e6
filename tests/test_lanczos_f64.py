"""The Lanczos-3 family against an independent float64 statement (tests/lanczos_f64.py).

Every bit-exact GPU test of the family builds its expectation from oracle/ref_kernels.c::orc_lanczos_bgra, which was written from the same
formula as the product's table builder.  Here the float64 statement is checked against closed forms (a), the oracle — over the shapes and the
content of the GPU modules, and the expectations those modules derive from it — against the statement (b), the statement against Pillow (c),
and wrong statements of the filter are shown to FAIL the comparison (d).  tests/test_gpu_lanczos_f64.py compares the kernels themselves."""
import functools

import numpy as np
import pytest

import lanczos_f64 as F
import test_gpu_lanczos_420 as T420
import test_gpu_lanczos_from_yuv as TF
import test_gpu_lanczos_ladder as TL
import test_gpu_lanczos_planar_ladder as TP
import test_gpu_lanczos_to_yuv as TT
import test_gpu_lanczos_yuv as TY
import util
from oracle import oracle as O


def ids(shapes):
    return ["%dx%d-%dx%d" % s for s in shapes]


# ---- a. the statement against closed forms: no oracle ---------------------------------------------------------------------------------------
AXES = [(16, 16), (36, 24), (33, 20), (17, 10), (64, 17), (600, 50), (100, 333), (2, 7), (1, 5), (5, 1), (220, 100)]


@pytest.mark.parametrize("n", [1, 2, 7, 16, 33])
def test_equal_sizes_give_the_identity(n):
    """(np.sinc of a non-zero integer is a few 1e-17, not 0)"""
    assert np.abs(F.matrix(n, n) - np.eye(n)).max() < 1e-15


@pytest.mark.parametrize("n_in,n_out", AXES)
def test_rows_sum_to_one_and_the_matrix_is_symmetric_about_the_centre(n_in, n_out):
    a, s, t = F.axis(n_in, n_out)
    assert a.shape == (n_out, n_in)
    assert np.abs(a.sum(axis=1) - 1.0).max() < 1e-14
    assert np.abs(a - a[::-1, ::-1]).max() < 1e-14          # A[o, i] == A[n_out - 1 - o, n_in - 1 - i]
    assert (s >= 1.0 - 1e-14).all() and s.max() < 1.6       # sum |w| of a normalised Lanczos-3
    fs = max(n_in / n_out, 1.0)
    assert 6 * fs - 2 <= t <= 6 * fs + 1                    # the samples strictly inside a support of 6 fs


def l3(t):
    """L3 written out once more, scalar"""
    if abs(t) >= 3:
        return 0.0
    if t == 0:
        return 1.0
    return np.sin(np.pi * t) / (np.pi * t) * np.sin(np.pi * t / 3) / (np.pi * t / 3)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_integer_enlargement_of_an_impulse(k):
    """background 64, impulse 192 at i0: out[o] = 64 + 128 L3((o + 0.5) / k - 0.5 - i0) / (sum of L3 over that row's integers); no lobe clips.
    The phases, by hand: k = 2 gives t = -0.25 and +0.25 around the impulse and steps of 0.5; k = 3 gives -1/3, 0, +1/3; k = 4 gives
    -0.375, -0.125, +0.125, +0.375"""
    n, i0 = 24, 11
    img = np.full((1, n), 64.0)
    img[0, i0] = 192.0
    out = F.resample(img, n * k, 1)[0]
    near = {2: [-0.25, 0.25], 3: [-1 / 3, 0.0, 1 / 3], 4: [-0.375, -0.125, 0.125, 0.375]}[k]
    for j, t0 in enumerate(near):
        assert abs(((k * i0 + j) + 0.5) / k - 0.5 - i0 - t0) < 1e-12
    for o in range(n * k):
        t = (o + 0.5) / k - 0.5 - i0                       # the impulse's distance from this output sample's centre
        row = sum(l3(i - ((o + 0.5) / k - 0.5)) for i in range(-8, n + 8))
        assert abs(out[o] - (64.0 + 128.0 * l3(-t) / row)) < 1e-10, (o, t)
    assert out.max() < 192.5 and out.min() > 40.0           # nothing near a clip


def test_two_to_one_reduction_of_an_impulse():
    """2:1: the kernel is twice as wide, so the impulse is seen at half-integer spacing: t = (i0 - c) / 2 with c = 2 o + 0.5"""
    n, i0 = 48, 23
    img = np.full((1, n), 64.0)
    img[0, i0] = 192.0
    out = F.resample(img, n // 2, 1)[0]
    for o in range(n // 2):
        c = 2 * o + 0.5
        row = sum(l3((i - c) / 2) for i in range(-16, n + 16))
        assert abs(out[o] - (64.0 + 128.0 * l3((i0 - c) / 2) / row)) < 1e-10, o
    # o = 11: c = 22.5, t = 0.25; o = 12: c = 24.5, t = -0.75; twelve samples inside the support on every row
    assert abs(out[11] - (64.0 + 128.0 * l3(0.25) / sum(l3((i - 22.5) / 2) for i in range(16, 30)))) < 1e-10
    assert F.axis(n, n // 2)[2] == 12


def test_the_axes_are_not_exchangeable():
    """33 x 17 -> 20 x 10 against the transposed problem: the picture's transpose resampled to 10 x 20 is the transpose of the result, and the
    same picture resampled with the axes' matrices exchanged is something else"""
    img = util.splitmix_bytes(5, 17 * 33).reshape(17, 33)
    v = F.resample(img, 20, 10)
    assert np.abs(F.resample(img.T.copy(), 10, 20) - v.T).max() < 1e-10
    ax, ay = F.matrix(33, 20), F.matrix(17, 10)
    assert np.abs(ay @ img @ ax.T - v).max() < 1e-10
    wrong = F.resample(img, 20, 10, x=exchange(17, 10), y=exchange(33, 20))
    assert np.abs(wrong - v).max() > 4.0


def test_weights_outside_the_picture_fold_onto_the_edge():
    """1 -> 5: every weight lands on the one sample; 2 -> 7: row 0 carries everything left of sample 0 on sample 0"""
    assert np.abs(F.matrix(1, 5) - 1.0).max() < 1e-14
    w, i = F.weights(2, 7)
    assert i.min() < 0 and i.max() > 1 and (np.abs(w[:, i < 0]).sum() > 0.05)
    a = F.matrix(2, 7)
    assert np.abs(a[:, 0] - w[:, i <= 0].sum(axis=1)).max() < 1e-15


# ---- b. the oracle against the statement ------------------------------------------------------------------------------------------------------
def ladder_shapes(*ladders):
    return [(*src, *size) for src, sizes in ladders for size in sizes]


LISTS = [TY.SHAPES, TY.VECTOR_ROW_SHAPES, TY.LAYOUT_SHAPES, TT.FIRST, TT.OTHERS, TT.LAYOUT_SHAPES, TF.SHAPES, TF.LAYOUT_SHAPES, T420.SHAPES,
         T420.LAYOUT_SHAPES, ladder_shapes(*TL.LADDERS.values()), ladder_shapes((TL.SRC, list(TL.RUNGS))), ladder_shapes(*TP.LADDERS.values()),
         ladder_shapes((TP.SRC, list(TP.RUNGS))), ladder_shapes((T420.SRC, T420.STRIP), (T420.SRC, T420.MIXED))]
SHAPES = sorted({tuple(s) for shapes in LISTS for s in shapes if tuple(s[:2]) != (1920, 1080)})
KINDS = ["random", "blocks"]
REFUSED = []           # what the oracle refuses (it returns non-zero): the only shapes a comparison may skip


def test_the_union_of_the_named_shapes():
    assert len(SHAPES) >= 40 and all(len(s) == 4 for s in SHAPES)
    for must in [(36, 20, 24, 14), (600, 64, 50, 8), (33, 17, 20, 10), (100, 50, 333, 171), (1, 1, 5, 3), (5, 3, 1, 1), (288, 144, 82, 41), (1100, 40, 367, 13)]:
        assert must in SHAPES, must
    assert not any(1080 in s for s in SHAPES)


def source4(kind, iw, ih, ow, oh):
    """(seeded as the GPU modules seed their cases: iw * 7 + oh)"""
    if kind == "random":
        return util.alloc_image("bgra", iw, ih, seed=iw * 7 + oh)[0]
    rng = np.random.default_rng(iw * 7 + oh)
    return np.ascontiguousarray(np.stack([TF.blocks(rng, ih, iw, (0, 255, 16, 235)) for _ in range(4)], axis=-1))


@functools.lru_cache(maxsize=None)
def plane4(kind, iw, ih, ow, oh):
    """(the oracle's codes or None where it refuses, the float64 Plane) of one 4-component case"""
    src = source4(kind, iw, ih, ow, oh)
    d4 = np.zeros((oh, ow, 4), dtype=np.uint8)
    if O.lanczos_bgra(d4, src, threads=4) != 0:
        return None, None
    return d4, F.Plane(src, ow, oh)


def picture(kind, iw, ih, ow, oh):
    if kind == "random":
        return util.alloc_image("nv12", iw, ih, seed=iw * 7 + oh)
    rng = np.random.default_rng(iw * 7 + oh)
    cw, ch = TF.chroma_size(iw, ih)
    return [TF.blocks(rng, ih, iw, (0, 255, 16, 235)), np.ascontiguousarray(np.stack([TF.blocks(rng, ch, cw, (0, 255, 16, 240)) for _ in range(2)], axis=-1))]


@functools.lru_cache(maxsize=None)
def planes_nv12(kind, iw, ih, ow, oh):
    """[(the oracle's plane through the 1- and 2-channel construction of tests/test_gpu_lanczos_yuv.py, the float64 Plane of that plane)]"""
    src = picture(kind, iw, ih, ow, oh)
    exp = TY.reference("nv12", src, iw, ih, ow, oh)
    return [(e, F.Plane(np.asarray(s), *np.shape(e)[1::-1])) for s, e in zip(src, exp)]


def check_plain(shape, kind, shares):
    codes, ref = plane4(kind, *shape)
    if codes is None:
        if shape not in REFUSED:
            REFUSED.append(shape)
        return []
    rows = []
    what = "%dx%d -> %dx%d, %s" % (*shape, kind)
    F.assert_plain(ref, codes, "oracle, 4 components, " + what)
    shares.add(ref.undecided, ref.v.shape[0] * ref.v.shape[1], "4 components, " + what)
    rows.append(ref.looseness(codes))
    for k, (e, p) in enumerate(planes_nv12(kind, *shape)):
        F.assert_plain(p, e, f"oracle, nv12 plane {k}, " + what)
        shares.add(p.undecided, p.v.shape[0] * p.v.shape[1], f"nv12 plane {k}, " + what)
        rows.append(p.looseness(e))
    return rows


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_oracle_plain_resample(shape, kind):
    """orc_lanczos_bgra on a 4-component plane, and on the planes of an NV12 picture each at its own size: every code within 0.5 + delta of
    the float64 value, no sample left out; planes of 400 samples or more hold the 2 % cap on undecided samples"""
    rows = check_plain(shape, kind, F.Shares(F.PLAIN_CAP))
    assert rows or shape in REFUSED
    for worst, d in rows:
        assert worst <= d


def test_oracle_refuses_nothing_and_the_small_planes_hold_the_cap_together():
    """the planes of fewer than 400 samples, pooled; and no shape of the union is skipped: the oracle refuses none of them today"""
    shares = F.Shares(F.PLAIN_CAP)
    for shape in SHAPES:
        for kind in KINDS:
            check_plain(shape, kind, shares)
    assert REFUSED == []
    assert shares.pool_n > 1000
    shares.assert_pool("orc_lanczos_bgra, planes below 400 samples")


FROM_SHAPES = [s for s in TF.SHAPES if s[:2] != (1920, 1080)]
TO_SHAPES = [s for s in TT.FIRST + TT.OTHERS if s[:2] != (1920, 1080)]


@functools.lru_cache(maxsize=None)
def from_yuv_planes(shape, kind):
    (y, cb, cr), _ = TF.case(*shape, kind)
    return tuple(F.Plane(p, *shape[2:]) for p in (y, cb, cr))


def check_from_yuv(shape, kind, shares):
    (y, cb, cr), cod = TF.case(*shape, kind)
    ref = from_yuv_planes(shape, kind)
    for name, p, c in zip(("Y", "Cb", "Cr"), ref, cod):
        F.assert_plain(p, c, "from_yuv's %s codes, %dx%d -> %dx%d, %s" % (name, *shape, kind))
    for sfmt in TF.SOURCES:
        for dfmt in TF.TARGETS:
            for csc in range(4):
                exp = TF.expected(sfmt, TF.packed(sfmt, y, cb, cr), *shape[2:], dfmt, csc)[0]
                lo, hi = F.from_yuv_interval(csc, dfmt, *ref)
                F.assert_within(lo, hi, exp, "%s -> %s, colourspace %d, %dx%d -> %dx%d, %s" % (sfmt, dfmt, csc, *shape, kind))
                assert (exp[..., 3] == 255).all()
                if sfmt == TF.SOURCES[0]:
                    shares.add((lo != hi)[..., :3], shape[2] * shape[3], "from_yuv %s colourspace %d, %dx%d -> %dx%d, %s" % (dfmt, csc, *shape, kind))


@pytest.mark.parametrize("kind", TF.KINDS)
@pytest.mark.parametrize("shape", FROM_SHAPES, ids=ids(FROM_SHAPES))
def test_from_yuv_expectation_lies_in_the_interval(shape, kind):
    """tests/test_gpu_lanczos_from_yuv.py::expected — both packings, both orders, every colourspace — inside [f(lo ...), f(hi ...)];
    at most 5 % of a target's colour bytes are left undecided (the alpha bytes, always 255, are not counted)"""
    check_from_yuv(shape, kind, F.Shares(F.MATRIX_CAP))


def check_to_yuv(shape, kind, shares):
    seed = shape[0] * 7 + shape[3]
    src, codes = TT.lanczos_codes(kind, *shape, seed)
    ref = to_yuv_plane(shape, kind)
    F.assert_plain(ref, codes, "to_yuv's codes, %dx%d -> %dx%d, %s" % (*shape, kind))
    for fmt in TT.FORMATS:
        for order in TT.ORDERS:
            for csc in range(4):
                _, exp = TT.expected(fmt, order, kind, *shape, seed, csc)
                exp = TF.logical(fmt, exp)
                for name, (lo, hi), e in zip(("Y", "Cb", "Cr"), F.to_yuv_interval(csc, order, ref), exp):
                    what = "%s %s -> %s, colourspace %d, %dx%d -> %dx%d, %s" % (name, order, fmt, csc, *shape, kind)
                    F.assert_within(lo, hi, e, what)
                    if fmt == TT.FORMATS[0]:
                        shares.add(lo != hi, lo.size, "to_yuv " + what)


@functools.lru_cache(maxsize=None)
def to_yuv_plane(shape, kind):
    src, _ = TT.lanczos_codes(kind, *shape, shape[0] * 7 + shape[3])
    return F.Plane(src, *shape[2:])


@pytest.mark.parametrize("kind", ["random", "blocks"])
@pytest.mark.parametrize("shape", TO_SHAPES, ids=ids(TO_SHAPES))
def test_to_yuv_expectation_lies_in_the_interval(shape, kind):
    """tests/test_gpu_lanczos_to_yuv.py::expected — both packings, both orders, every colourspace — plane by plane inside the interval that
    section 4.4.2's integer arithmetic makes of [lo, hi]; at most 5 % of a plane's bytes undecided"""
    check_to_yuv(shape, kind, F.Shares(F.MATRIX_CAP))


def test_the_small_planes_behind_a_matrix_hold_the_cap_together():
    shares = F.Shares(F.MATRIX_CAP)
    for kind in TF.KINDS:
        for shape in FROM_SHAPES:
            check_from_yuv(shape, kind, shares)
    for kind in ["random", "blocks"]:
        for shape in TO_SHAPES:
            check_to_yuv(shape, kind, shares)
    assert shares.pool_n > 1000
    shares.assert_pool("from_yuv and to_yuv expectations, planes below 400 samples")


def test_the_tables_written_out_in_the_statement_are_the_gpu_modules():
    """lanczos_f64 carries sections 4.2 and 4.5 from DESIGN.md; the GPU modules carry them too (from_yuv's written out, to_yuv's rebuilt from the
    luma weights in rational arithmetic): three statements, one table"""
    assert F.YUV_TO_RGB == TF.CSC
    for csc in range(4):
        assert F.RGB_TO_YUV[csc] == TT.tables(csc)


# ---- c. Pillow as a third opinion ---------------------------------------------------------------------------------------------------------------
PILLOW_SHAPES = [(100, 50, 333, 171), (64, 36, 128, 72), (440, 220, 200, 100), (256, 128, 128, 64), (700, 140, 200, 40), (146, 40, 73, 20)]


def interior(n_in, n_out):
    """the output samples whose whole support lies inside the picture: Pillow renormalises at an edge where section 4.4 clamps"""
    w, i = F.weights(n_in, n_out)
    touched = w != 0.0
    first, last = i[np.argmax(touched, axis=1)], i[touched.shape[1] - 1 - np.argmax(touched[:, ::-1], axis=1)]
    return (first >= 1) & (last <= n_in - 2)


@pytest.mark.parametrize("shape", PILLOW_SHAPES, ids=ids(PILLOW_SHAPES))
def test_pillow_agrees_in_the_interior(shape):
    """Image.resize(..., Image.LANCZOS) on mode "L": code nobody here wrote, with the same sampling convention (pixel centres, a kernel widened
    on reduction).  Pillow resamples horizontally, rounds to 8 bits, resamples vertically and rounds again, with coefficients rounded to 22
    fractional bits: against the unrounded float64 value that is 0.5 for the last rounding, 0.5 max S_y for the first one carried through the
    vertical pass, and 2^-23 per coefficient on values up to 255 (T = T_x + T_y coefficients; S_y < 2): 0.5 + 0.5 max S_y + 255 T 2^-22.
    Content stays within codes 80 .. 175 so that the 8-bit intermediate cannot clip."""
    Image = pytest.importorskip("PIL.Image")
    iw, ih, ow, oh = shape
    img = (80 + util.splitmix_bytes(iw * 3 + oh, iw * ih).reshape(ih, iw) % 96).astype(np.uint8)
    assert img.min() >= 80 and img.max() <= 175
    assert Image.fromarray(img).mode == "L"
    got = np.asarray(Image.fromarray(img).resize((ow, oh), Image.LANCZOS)).astype(np.float64)
    v = F.resample(img, ow, oh)
    (_, _, tx), (_, sy, ty) = F.axis(iw, ow), F.axis(ih, oh)
    assert sy.max() < 2.0
    tol = 0.5 + 0.5 * sy.max() + 255.0 * (tx + ty) * 2.0 ** -22
    inside = interior(ih, oh)[:, None] & interior(iw, ow)[None, :]
    assert inside.sum() >= 0.5 * inside.size, "too little of the picture is interior to mean anything"
    worst = np.abs(got - v)[inside].max()
    print("pillow %dx%d -> %dx%d: interior %d of %d, worst |pillow - v| %.3f, tolerance %.3f" % (*shape, inside.sum(), inside.size, worst, tol))
    assert worst <= tol
    # and the comparison can fail: against a statement without the -0.5 it does, on most samples
    off = F.resample(img, ow, oh, centre=lambda o, n_in, n_out: (o + 0.5) * n_in / n_out)
    assert (np.abs(got - off)[inside] > tol).mean() > 0.5


# ---- d. teeth: wrong statements of the filter fail the comparison -------------------------------------------------------------------------------
def exchange(n_in, n_out):
    """an axis that takes its centres and its width from another axis's sizes"""
    return dict(centre=lambda o, _i, _o: F.centre(o, n_in, n_out), width=lambda _i, _o: F.width(n_in, n_out))


def whole(**how):
    return lambda iw, ih, ow, oh: dict(how)


WRONG = {
    "a=2 window": whole(kernel=lambda t: np.where(np.abs(t) < 3.0, np.sinc(t) * np.sinc(np.asarray(t) / 2.0), 0.0)),
    "centre without -0.5": whole(centre=lambda o, n_in, n_out: (o + 0.5) * n_in / n_out),
    "no widening on reduction": whole(width=lambda n_in, n_out: 1.0),
    "corner-aligned centres": whole(centre=lambda o, n_in, n_out: o * (n_in - 1) / max(n_out - 1, 1)),
    "first shifted by one": whole(centre=lambda o, n_in, n_out: F.centre(o, n_in, n_out) + 1.0),
    "x and y exchanged": lambda iw, ih, ow, oh: dict(x=exchange(ih, oh), y=exchange(iw, ow)),
}
TEETH_SHAPES = [(36, 20, 24, 14), (33, 17, 20, 10), (440, 220, 200, 100), (64, 36, 17, 9), (100, 50, 333, 171)]
# where a wrong statement says the same as the right one, the comparison passes: the variants are wrong, not noisy
EQUIVALENT = {"no widening on reduction": (100, 50, 333, 171),          # an enlargement has nothing to widen
              "x and y exchanged": (440, 220, 200, 100)}               # both axes 2.2 : 1


def failing_share(codes, wrong, right):
    """the share of samples at which the codes leave 0.5 + delta around the wrong statement's value (delta: the right statement's)"""
    return float((np.abs(codes.astype(np.float64) - np.clip(wrong, 0.0, 255.0)) - 0.5 - right.d > 0.0).mean())


@pytest.mark.parametrize("name", list(WRONG))
def test_a_wrong_statement_fails_against_the_oracle(name):
    shares = {}
    for shape in TEETH_SHAPES:
        codes, right = plane4("random", *shape)
        wrong = F.resample(source4("random", *shape), *shape[2:], **WRONG[name](*shape))
        shares[shape] = failing_share(codes, wrong, right)
    best = max(shares, key=shares.get)
    print("%s: caught on %dx%d -> %dx%d with %.1f %% of the samples failing; all: %s" %
          (name, *best, 100 * shares[best], {"%dx%d-%dx%d" % s: round(100 * v, 1) for s, v in shares.items()}))
    assert shares[best] > 0.5
    if name == "x and y exchanged":
        assert shares[(33, 17, 20, 10)] > 0.5                 # 1.65 : 1 against 1.7 : 1
    if name in EQUIVALENT:
        assert shares[EQUIVALENT[name]] == 0.0


def test_chroma_resampled_with_the_luma_matrices_fails_against_the_oracle():
    """33 x 17 -> 20 x 10: chroma is 16 x 8 -> 10 x 5 (1.6 : 1), luma 1.65 : 1 and 1.7 : 1.  At 256 x 128 -> 128 x 64 every plane is 2 : 1 and
    the mistake says the same as the right statement."""
    shares = {}
    for shape in [(33, 17, 20, 10), (36, 20, 24, 14), (256, 128, 128, 64)]:
        iw, ih, ow, oh = shape
        e, right = planes_nv12("random", *shape)[1]
        wrong = F.resample(picture("random", *shape)[1], *np.shape(e)[1::-1], x=exchange(iw, ow), y=exchange(ih, oh))
        shares[shape] = failing_share(e, wrong, right)
    print("chroma with the luma matrices: %s" % {"%dx%d-%dx%d" % s: round(100 * v, 1) for s, v in shares.items()})
    assert shares[(33, 17, 20, 10)] > 0.5
    assert shares[(256, 128, 128, 64)] == 0.0


def test_the_right_statement_passes_where_the_wrong_ones_fail():
    for shape in TEETH_SHAPES:
        codes, right = plane4("random", *shape)
        assert failing_share(codes, right.v, right) == 0.0
