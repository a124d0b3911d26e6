"""chv_scale_lanczos_420 / chv_scale_lanczos_420_ladder: Lanczos-3 between NV12 and y420p pictures.  Bit-exact, no
tolerance, no case excluded.

The call resamples the logical planes Y, Cb and Cr one by one and stores them in the target's packing, so the expected bytes are the same-format
reference of tests/test_gpu_lanczos_yuv.py (the oracle's 4-channel Lanczos, plane by plane, cached) of the SOURCE's format, repacked here in
numpy.  Every target is pre-filled with seeded bytes and whole planes are compared."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gpuutil as G
import layouts as L
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv
from test_gpu_lanczos_yuv import FORMATS, Placing, case, random_geometry, reference

pytestmark = pytest.mark.gpu

K = sv.defaultComputeKernelFromString
NP = {"nv12": 2, "y420p": 3}
CROSS = [("nv12", "y420p"), ("y420p", "nv12")]
PAIR_IDS = ["nv12-to-y420p", "y420p-to-nv12"]


def repack(planes, sfmt, dfmt):
    """the planes of a picture of packing `sfmt` as the planes of the same picture in packing `dfmt` (fresh arrays)"""
    if sfmt == dfmt:
        return [np.array(p, copy=True) for p in planes]
    if dfmt == "y420p":
        return [np.array(planes[0], copy=True), planes[1][..., 0].copy(), planes[1][..., 1].copy()]
    return [np.array(planes[0], copy=True), np.stack([planes[1], planes[2]], axis=-1)]


def xcase(sfmt, dfmt, iw, ih, ow, oh, seed):
    """(source planes in sfmt, expected planes in dfmt) from the shared, cached same-format reference"""
    src, exp = case(sfmt, iw, ih, ow, oh, seed)
    return src, repack(exp, sfmt, dfmt)


def counter():
    return cv.get_counter("lanczos_420_ladder_launches")


def run_single(ctx, sfmt, dfmt, iw, ih, ow, oh, seed, what=""):
    src, exp = xcase(sfmt, dfmt, iw, ih, ow, oh, seed)
    gs = G.to_gpu(ctx, sfmt, iw, ih, src)
    gd = G.to_gpu(ctx, dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=seed + 7))
    sv.usingContext(ctx, lambda c: sv.scaleLanczos420(c, gd, gs))
    G.assert_same(G.from_gpu(ctx, gd, dfmt, ow, oh), exp, f"{sfmt} -> {dfmt} lanczos {iw}x{ih} -> {ow}x{oh} {what}")


# ---- 1. named shapes ------------------------------------------------------------------------------------------------------------------
SHAPES = [(16, 16, 16, 16),
          (36, 20, 24, 14),
          (146, 20, 73, 10),         # 12 luma / 14 chroma taps
          (33, 17, 20, 10),          # odd sizes, tap counts differ per axis
          (8, 8, 5, 5),              # a chroma row shorter than a dword
          (2, 2, 7, 5),              # 1 x 1 chroma
          (100, 50, 333, 171),       # enlargement, six NV12 chroma strips
          (256, 128, 128, 64),       # rows of whole vectors: the hand-awaited path on both chroma planes
          (700, 140, 200, 40),       # 22 taps, the longest staged row
          (64, 36, 17, 9),           # 24 taps, tile route
          (1100, 40, 550, 20),       # partial last strip
          (1000, 200, 500, 100)]     # row chunks with a short tail


@pytest.mark.parametrize("sfmt,dfmt", CROSS, ids=PAIR_IDS)
@pytest.mark.parametrize("iw,ih,ow,oh", SHAPES)
def test_named_shapes(ctx, sfmt, dfmt, iw, ih, ow, oh):
    run_single(ctx, sfmt, dfmt, iw, ih, ow, oh, seed=iw * 7 + oh)


# ---- 2. first principles: at equal sizes the call is an exact repack (no oracle) ------------------------------------------------------------
@pytest.mark.parametrize("sfmt,dfmt", CROSS, ids=PAIR_IDS)
@pytest.mark.parametrize("w,h", [(64, 36), (130, 20), (7, 5), (2, 2)])
def test_equal_sizes_repack_exactly(ctx, sfmt, dfmt, w, h):
    """6 taps per axis at 1:1, the centre weight 1 and the others 0 after rounding to float: every logical plane comes out as it went in"""
    src = util.alloc_image(sfmt, w, h, seed=w * 31 + h)
    gs = G.to_gpu(ctx, sfmt, w, h, src)
    gd = G.to_gpu(ctx, dfmt, w, h, util.alloc_image(dfmt, w, h, seed=5))
    sv.usingContext(ctx, lambda c: sv.scaleLanczos420(c, gd, gs))
    G.assert_same(G.from_gpu(ctx, gd, dfmt, w, h), repack(src, sfmt, dfmt), f"{sfmt} -> {dfmt} repack at {w}x{h}")


# ---- 3. same-format pairs through the new entries are chv_scale_lanczos's ---------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("iw,ih,ow,oh", [(36, 20, 24, 14), (146, 20, 73, 10), (64, 36, 17, 9)])
def test_same_format_pairs_equal_scale_lanczos(ctx, fmt, iw, ih, ow, oh):
    src, exp = case(fmt, iw, ih, ow, oh, iw * 7 + oh)
    gs = G.to_gpu(ctx, fmt, iw, ih, src)
    a, b, l = (G.to_gpu(ctx, fmt, ow, oh, util.alloc_image(fmt, ow, oh, seed=s)) for s in (3, 4, 5))
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczos420(c, a, gs))
    sv.usingContext(ctx, lambda c: sv.scaleLanczos420Ladder(c, [[l]], [gs]))
    assert counter() == before, "a same-format pair is forwarded: the cross path launched nothing"
    sv.usingContext(ctx, lambda c: sv.scaleLanczos(c, b, gs))
    want = G.from_gpu(ctx, b, fmt, ow, oh)
    G.assert_same(want, exp, "chv_scale_lanczos against the reference")
    G.assert_same(G.from_gpu(ctx, a, fmt, ow, oh), want, f"{fmt} -> {fmt} through chv_scale_lanczos_420")
    G.assert_same(G.from_gpu(ctx, l, fmt, ow, oh), want, f"{fmt} -> {fmt} through chv_scale_lanczos_420_ladder")


# ---- 4. random geometries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(16))
def test_random_geometries(ctx, seed):
    """the generator and bounds of tests/test_gpu_lanczos_yuv.py: every draw must succeed"""
    iw, ih, ow, oh = random_geometry(seed)
    sfmt, dfmt = CROSS[seed % 2]
    run_single(ctx, sfmt, dfmt, iw, ih, ow, oh, seed=seed + 1)


# ---- 5. foreign layouts ----------------------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(36, 20, 24, 14), (146, 20, 73, 10), (8, 8, 5, 5), (256, 128, 128, 64)]


@pytest.fixture
def placing(ctx):
    p = Placing(ctx)
    yield p
    p.rec.sweep(ctx)            # every allocation downloaded completely: payload of the targets changed, nothing else, no byte of a source


@pytest.mark.parametrize("sfmt,dfmt", CROSS, ids=PAIR_IDS)
@pytest.mark.parametrize("iw,ih,ow,oh", LAYOUT_SHAPES)
@pytest.mark.parametrize("layout", L.LAYOUTS)
def test_foreign_layouts(ctx, placing, sfmt, dfmt, iw, ih, ow, oh, layout):
    src, exp = xcase(sfmt, dfmt, iw, ih, ow, oh, iw * 7 + oh)
    gs = placing.place(sfmt, iw, ih, src, layout)
    gd = placing.place(dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=11), layout)
    sv.usingContext(ctx, lambda c: sv.scaleLanczos420(c, gd, gs))
    G.assert_same(placing.from_gpu(gd, dfmt, ow, oh), exp, f"{sfmt} -> {dfmt} lanczos {iw}x{ih} -> {ow}x{oh} on {layout}")


@pytest.mark.parametrize("aligned_plane", [1, 2])
@pytest.mark.parametrize("iw,ih,ow,oh", [(256, 128, 128, 64), (146, 20, 73, 10)])
def test_y420p_source_with_one_vector_aligned_chroma_plane(ctx, placing, iw, ih, ow, oh, aligned_plane):
    """Cb at a 16-byte address and pitch and Cr at an odd byte (and the other way round): the hand-awaited path needs BOTH planes, the
    compiler-managed one takes vectors from the plane that has them and gathers the other.  The picture is put together from the planes of
    two placed copies of one source."""
    src, exp = xcase("y420p", "nv12", iw, ih, ow, oh, iw * 7 + oh)
    good, odd = placing.place("y420p", iw, ih, src, "guarded"), placing.place("y420p", iw, ih, src, "skewed")
    pg, po = placing.rec.placement(good), placing.rec.placement(odd)
    assert pg.planes[aligned_plane].aligned16() and po.planes[3 - aligned_plane].offset % 2 == 1
    pick = [good, good, good]
    pick[3 - aligned_plane] = odd
    bufs = [s.imageBuffer() for s in pick]
    plans = [pg if s is good else po for s in pick]
    img = good.imageBuffer().withChanges(computeTextures=[b.computeTextures[p] for p, b in enumerate(bufs)],
                                         gpuPitches=[pl.planes[p].pitch for p, pl in enumerate(plans)],
                                         gpuOffsets=[pl.planes[p].offset for p, pl in enumerate(plans)])
    gs = sv.PictureSample(img)
    gd = placing.place("nv12", ow, oh, util.alloc_image("nv12", ow, oh, seed=11), "guarded")
    sv.usingContext(ctx, lambda c: sv.scaleLanczos420(c, gd, gs))
    G.assert_same(placing.from_gpu(gd, "nv12", ow, oh), exp, f"y420p -> nv12 {iw}x{ih} -> {ow}x{oh}, only plane {aligned_plane} of the chroma planes aligned")


# ---- 6. ladders ------------------------------------------------------------------------------------------------------------------------
SRC = (288, 144)
STRIP = [(240, 120), (191, 95), (96, 48)]             # 8 taps, 10 (odd: floor'd chroma), 18: the four-wave variant
MIXED = [(144, 72), (72, 36), (96, 48)]               # the middle one: 24 taps, the tile route


def references(sfmt, dfmt, src_size, sizes, n):
    iw, ih = src_size
    srcs, exps = [None] * n, [[None] * n for _ in sizes]
    for r, (w, h) in enumerate(sizes):
        for i in range(n):
            srcs[i], exps[r][i] = xcase(sfmt, dfmt, iw, ih, w, h, 900 + i)
    return srcs, exps


def fresh_targets(ctx, fmt, sizes, n, seed):
    return [[G.to_gpu(ctx, fmt, w, h, util.alloc_image(fmt, w, h, seed=seed + 16 * r + i)) for i in range(n)] for r, (w, h) in enumerate(sizes)]


def check_rungs(ctx, fmt, sizes, rungs, exps, what, singles=None):
    for r, (w, h) in enumerate(sizes):
        for i, gd in enumerate(rungs[r]):
            got = G.from_gpu(ctx, gd, fmt, w, h)
            G.assert_same(got, exps[r][i], f"{what}: rung {r} ({w}x{h}) of source {i} against the reference")
            if singles:
                G.assert_same(got, G.from_gpu(ctx, singles[r][i], fmt, w, h), f"{what}: rung {r} ({w}x{h}) of source {i} against the single call")


@pytest.mark.parametrize("sfmt,dfmt", CROSS, ids=PAIR_IDS)
@pytest.mark.parametrize("name,sizes,launches", [("strip", STRIP, 1), ("mixed", MIXED, 2)])
def test_ladder_of_five_pictures(ctx, sfmt, dfmt, name, sizes, launches):
    """three rungs of five pictures; with a tile rung exactly two launches by the counter"""
    srcs, exps = references(sfmt, dfmt, SRC, sizes, 5)
    gs = [G.to_gpu(ctx, sfmt, *SRC, s) for s in srcs]
    rungs = fresh_targets(ctx, dfmt, sizes, 5, 3)
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczos420Ladder(c, rungs, gs))
    assert counter() - before == launches
    check_rungs(ctx, dfmt, sizes, rungs, exps, f"{name} ladder {sfmt} -> {dfmt}")


def header_chunk(n_rungs, dst_planes, src_planes):
    """CHV_420_LADDER_CHUNK of include/chipvideo.h, from the header's own text and numbers"""
    text = (Path(__file__).resolve().parents[1] / "include" / "chipvideo.h").read_text()
    slot = int(re.search(r"#define CHV_LADDER_SLOT_BYTES (\d+)", text).group(1))
    plane = int(re.search(r"#define CHV_LADDER_PLANE_BYTES (\d+)", text).group(1))
    assert ("#define CHV_420_LADDER_CHUNK(n_rungs, dst_planes, src_planes) (CHV_LADDER_SLOT_BYTES / (((n_rungs) * (dst_planes) + (src_planes)) * "
            "CHV_LADDER_PLANE_BYTES))") in text
    return slot // ((n_rungs * dst_planes + src_planes) * plane)


@pytest.mark.parametrize("sfmt,dfmt", CROSS, ids=PAIR_IDS)
def test_eight_rungs_one_picture_more_than_a_chunk(ctx, sfmt, dfmt):
    """two chunks; the last rung takes the tile route: two launches per chunk, all rungs of a picture in one chunk"""
    src_size = (40, 24)
    sizes = [(40, 24), (56, 30), (36, 20), (30, 18), (27, 15), (24, 14), (20, 12), (10, 6)]
    n = header_chunk(8, NP[dfmt], NP[sfmt]) + 1
    assert 2 < n < 20
    srcs, exps = references(sfmt, dfmt, src_size, sizes, n)
    gs = [G.to_gpu(ctx, sfmt, *src_size, s) for s in srcs]
    rungs = fresh_targets(ctx, dfmt, sizes, n, 7)
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczos420Ladder(c, rungs, gs))
    assert counter() - before == 4
    check_rungs(ctx, dfmt, sizes, rungs, exps, f"{n} pictures, eight rungs, {sfmt} -> {dfmt}")


@pytest.mark.parametrize("sfmt,dfmt", CROSS, ids=PAIR_IDS)
def test_one_rung_of_n_equals_n_single_calls(ctx, sfmt, dfmt):
    sizes, n = [(191, 95)], 4
    srcs, exps = references(sfmt, dfmt, SRC, sizes, n)
    gs = [G.to_gpu(ctx, sfmt, *SRC, s) for s in srcs]
    rungs, singles = fresh_targets(ctx, dfmt, sizes, n, 9), fresh_targets(ctx, dfmt, sizes, n, 1009)
    ladder = sv.Lanczos420Ladder(rungs, gs)
    sv.usingContext(ctx, lambda c: ladder.run(c))
    for i in range(n):
        sv.usingContext(ctx, lambda c: sv.scaleLanczos420(c, singles[0][i], gs[i]))
    check_rungs(ctx, dfmt, sizes, rungs, exps, f"one rung of {n}, {sfmt} -> {dfmt}", singles)


def test_empty_ladders_are_noops(ctx):
    before = counter()
    lib = cv.load()
    cv.check(lib.chv_scale_lanczos_420_ladder(ctx.handle, None, 0, None, 3))
    cv.check(lib.chv_scale_lanczos_420_ladder(ctx.handle, None, 3, None, 0))
    assert sv.scaleLanczos420Ladder(ctx, [], []) is ctx
    assert counter() == before


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------
class Pictures:
    """targets and sources with the bytes they were filled with, so that every one of them can be shown unchanged afterwards"""

    def __init__(self, ctx):
        self.ctx, self.made, self.seed = ctx, [], 100

    def __call__(self, fmt, w, h):
        self.seed += 1
        planes = util.alloc_image(fmt, w, h, seed=self.seed)
        g = G.to_gpu(self.ctx, fmt, w, h, planes)
        self.made.append((g, fmt, w, h, planes))
        return g

    def unchanged(self, what):
        for g, fmt, w, h, planes in self.made:
            G.assert_same(G.from_gpu(self.ctx, g, fmt, w, h), planes, f"{what}: a refused call wrote to a {w}x{h} {fmt} picture")


def _case_of(rc):
    if rc == 0:
        return "success"
    with pytest.raises(sv.ComputeError) as e:
        cv.check(rc)
    return e.value.case


def single(ctx, d, s):
    return _case_of(cv.load().chv_scale_lanczos_420(ctx.handle, C.byref(d), C.byref(s)))


def ladder(ctx, rung_descs, src_descs):
    flat = [d for rung in rung_descs for d in rung]
    d, s = (cv.Image * len(flat))(*flat), (cv.Image * len(src_descs))(*src_descs)
    return _case_of(cv.load().chv_scale_lanczos_420_ladder(ctx.handle, d, len(rung_descs), s, len(src_descs)))


def test_errors_leave_every_target_unchanged(ctx):
    pic, desc = Pictures(ctx), sv._image_desc
    nv_s, yp_s, bg_s = pic("nv12", 64, 36), pic("y420p", 64, 36), pic("bgra", 64, 36)
    nv_d, yp_d, bg_d = pic("nv12", 32, 18), pic("y420p", 32, 18), pic("bgra", 32, 18)
    assert single(ctx, desc(bg_d), desc(nv_s)) == "badTarget"                   # a BGRA target
    assert single(ctx, desc(yp_d), desc(bg_s)) == "badInputData"                # a BGRA source
    assert ladder(ctx, [[desc(bg_d)]], [desc(nv_s)]) == "badTarget"
    assert ladder(ctx, [[desc(yp_d)]], [desc(bg_s)]) == "badInputData"
    for skew in ("width", "height"):                                            # a y420p picture with unequal chroma planes
        bad = desc(yp_d)
        setattr(bad.planes[2], skew, getattr(bad.planes[2], skew) - 1)
        assert single(ctx, bad, desc(nv_s)) == "badTarget"
        assert single(ctx, bad, desc(yp_s)) == "badTarget"                      # (also for the same-format pair, which chv_scale_lanczos would take)
        bad = desc(yp_s)
        setattr(bad.planes[1], skew, getattr(bad.planes[1], skew) - 1)
        assert single(ctx, desc(nv_d), bad) == "badInputData"
    far = desc(yp_d)                                                            # a plane extent outside its buffer
    far.planes[2].height = 1 << 20
    assert single(ctx, far, desc(nv_s)) == "badTarget"
    far = desc(yp_s)
    far.planes[1].offset = far.planes[1].offset + (1 << 30)
    assert single(ctx, desc(nv_d), far) == "badInputData"
    srcs = [desc(nv_s), desc(pic("nv12", 64, 36))]
    yp2, nv2 = pic("y420p", 32, 18), pic("nv12", 16, 10)
    assert ladder(ctx, [[desc(yp_d), desc(yp2)], [desc(nv2), desc(pic("y420p", 16, 10))]], srcs) == "invalidValue"     # mixed target formats
    assert ladder(ctx, [[desc(yp_d), desc(yp2)]], [desc(nv_s), desc(yp_s)]) == "invalidValue"                          # mixed source formats
    assert ladder(ctx, [[desc(yp_d), desc(pic("y420p", 30, 18))]], srcs) == "invalidValue"                             # two sizes inside a rung
    big, first, tiny = pic("nv12", 96, 96), pic("y420p", 48, 48), pic("y420p", 4, 4)                                   # 24:1: the 160 KB rule
    assert single(ctx, desc(tiny), desc(big)) == "invalidValue"
    assert ladder(ctx, [[desc(first)], [desc(tiny)]], [desc(big)]) == "invalidValue"                                   # refused in the LAST rung
    nine = [[desc(pic("y420p", 8 + 2 * r, 6))] for r in range(9)]
    assert ladder(ctx, nine, [desc(nv_s)]) == "invalidValue"
    with pytest.raises(sv.ComputeError) as e:                                   # a NULL list with non-zero counts
        cv.check(cv.load().chv_scale_lanczos_420_ladder(ctx.handle, None, 1, C.byref(desc(nv_s)), 1))
    assert e.value.case == "invalidValue"
    pic.unchanged("errors")
    # (the pictures the refusals were made from make good calls: every refusal above is the one it names)
    assert single(ctx, desc(yp_d), desc(nv_s)) == "success"
    assert single(ctx, desc(nv_d), desc(yp_s)) == "success"
    assert ladder(ctx, [[desc(first)]], [desc(big)]) == "success"


# ---- 8. inside a pass ------------------------------------------------------------------------------------------------------------------
def test_resize_inside_a_pass_sees_the_held_composite(ctx):
    cw, ch, ow, oh = 128, 72, 64, 36
    layer = util.alloc_image("bgra", 40, 30, seed=7)
    u = util.make_uniforms((cw, ch), rect=(10, 6, 60, 40), border=(2, 2, 2, 2), fill=(0.2, 0.6, 0.3, 0.7), opacity=0.8, in_size=(40, 30))
    canvas = util.alloc_image("nv12", cw, ch, seed=8)
    assert O.run_kernel("img_clear_nv12", canvas) == 0
    assert O.run_kernel("img_bgra_nv12", canvas, layer, u) == 0
    exp = repack(reference("nv12", canvas, cw, ch, ow, oh), "nv12", "y420p")
    gl = G.to_gpu(ctx, "bgra", 40, 30, layer)
    gc = G.to_gpu(ctx, "nv12", cw, ch, util.alloc_image("nv12", cw, ch, seed=8))
    gd = G.to_gpu(ctx, "y420p", ow, oh, util.alloc_image("y420p", ow, oh, seed=9))

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gc, kernel=K("img_clear_nv12"), blends=False)
        c = sv.runComputeKernel(c, images=[gl], target=gc, kernel=K("img_bgra_nv12"), uniforms=u, blends=True)
        c = sv.scaleLanczos420(c, gd, gc)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gc, "nv12", cw, ch), canvas, "the composited canvas")
    G.assert_same(G.from_gpu(ctx, gd, "y420p", ow, oh), exp, "the y420p rendition of the canvas composited in the same pass")


# ---- 9. PictureFilter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfmt,dfmt", CROSS, ids=PAIR_IDS)
def test_picture_filter_convert420(ctx, sfmt, dfmt):
    iw, ih, ow, oh = 96, 54, 64, 36
    src, exp = xcase(sfmt, dfmt, iw, ih, ow, oh, 41)
    f = sv.PictureFilter((ow, oh), G.FMT[dfmt], computeContext=ctx, scaler="lanczos", convert420=True)
    for sample in (sv.pictureFromArrays(G.FMT[sfmt], (iw, ih), src), G.to_gpu(ctx, sfmt, iw, ih, src)):
        kind, out = f(sample)
        assert kind == "just", out
        G.assert_same(G.from_gpu(f.context, out, dfmt, ow, oh), exp, f"PictureFilter lanczos {sfmt} -> {dfmt}")
