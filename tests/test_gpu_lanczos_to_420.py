"""chv_scale_lanczos_to_420 / chv_scale_lanczos_to_420_ladder: Lanczos-3 from the decoder's five other formats (nv21,
y422p, y444p, yuvs, zvuy) into NV12 and y420p pictures.  Bit-exact, no tolerance, no case excluded.

The cases — 321, three seconds together — are a TABLE run by one test (`cases()` at the end names them; the sections above are its
checks): they share sources, references and the C++ mirror's program, every case runs whether or not an earlier one failed, and the test
reports each failed case by its name.  Anything but a failed assertion — an error of the library or the runtime — ends the test at once.

The expected bytes are tests/decoder_formats.py's: every logical image (Y, Cb, Cr) of the source through the oracle's Lanczos on its own sizes,
stored in the target's packing.  Every target is pre-filled with seeded bytes and whole planes are compared."""
import ctypes as C

import numpy as np
import pytest

import decoder_formats as D
import gpuutil as G
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv
from test_gpu_lanczos_420 import Pictures, _case_of, check_rungs, fresh_targets, header_chunk
from test_gpu_lanczos_yuv import Placing

K = sv.defaultComputeKernelFromString
NP = {"nv12": 2, "y420p": 3}
CELLS = [(s, d) for s in D.FORMATS for d in D.TARGETS]
CELL_IDS = [f"{s}-to-{d}" for s, d in CELLS]


def counter():
    return cv.get_counter("lanczos_to_420_launches")


def run_single(ctx, sfmt, dfmt, iw, ih, ow, oh, seed, what=""):
    src, exp = D.case(sfmt, dfmt, iw, ih, ow, oh, seed)
    gs = D.to_gpu(ctx, sfmt, iw, ih, src)
    gd = G.to_gpu(ctx, dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=seed + 7))
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420(c, gd, gs))
    assert counter() - before == 1, "a single call takes one route: one launch"
    G.assert_same(G.from_gpu(ctx, gd, dfmt, ow, oh), exp, f"{sfmt} -> {dfmt} lanczos {iw}x{ih} -> {ow}x{oh} {what}")


# ---- 1. named shapes ------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 2, 2, 2), (2, 2, 4, 4),          # the smallest
          (34, 18, 34, 18),                    # equal sizes
          (66, 34, 40, 22),                    # a 4:4:4 chroma of 66 -> 20 is 20 taps, class 22
          (20, 10, 66, 34),                    # enlargement, a partial second strip
          (38, 18, 21, 11), (33, 17, 21, 11),  # odd targets: the last column and row own luma only
          (200, 12, 150, 8),                   # three strips per row
          (130, 40, 40, 12)]                   # tile route for 4:2:2 and 4:4:4, strip for NV21
TILE_130 = {"nv21": False, "y422p": True, "y444p": True, "yuvs": True, "zvuy": True}


def shape_cells():
    out = []
    for shape in SHAPES:
        for s, d in CELLS:
            if shape[0] % 2 and s in D.PACKED:
                continue                        # (a packed picture has an even width)
            out.append(pytest.param(s, d, *shape, id=f"{s}-to-{d}-{shape[0]}x{shape[1]}-{shape[2]}x{shape[3]}"))
    return out


def test_the_reference_accepts_every_named_shape_and_the_routes_are_the_expected_ones():
    """CPU only: the rules of tests/decoder_formats.py on the named shapes, before any of them runs"""
    for p in shape_cells():
        s, d, iw, ih, ow, oh = p.values
        assert not D.refused(s, d, iw, ih, ow, oh), p.id
        if (iw, ih, ow, oh) == (130, 40, 40, 12):
            assert D.strip_route(s, d, iw, ih, ow, oh) == (not TILE_130[s]), p.id
        elif max(iw / ow, ih / oh) <= 1.8:      # (at most 22 chroma taps even from 4:4:4; steeper shapes go where the rule sends them)
            assert D.strip_route(s, d, iw, ih, ow, oh), p.id
    assert D.taps(66, 20) == 20 and D.strip_route("y444p", "nv12", 66, 34, 40, 22) and D.strip_route("y444p", "y420p", 66, 34, 40, 22)


def check_named_shapes(ctx, sfmt, dfmt, iw, ih, ow, oh):
    run_single(ctx, sfmt, dfmt, iw, ih, ow, oh, seed=iw * 7 + oh)


# ---- 2. first principles at equal sizes: plain numpy indexing, no oracle ------------------------------------------------------------------
def equal_size_call(ctx, sfmt, dfmt, w, h):
    src = D.alloc(sfmt, w, h, seed=w * 31 + h)
    gs = D.to_gpu(ctx, sfmt, w, h, src)
    gd = G.to_gpu(ctx, dfmt, w, h, util.alloc_image(dfmt, w, h, seed=5))
    sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420(c, gd, gs))
    return src, G.from_gpu(ctx, gd, dfmt, w, h)


def check_equal_sizes_luma_is_the_sources(ctx, sfmt, dfmt, w, h):
    src, got = equal_size_call(ctx, sfmt, dfmt, w, h)
    if sfmt in D.PACKED:
        y = src[0].reshape(h, 2 * w)[:, (0 if sfmt == "yuvs" else 1)::2]
    else:
        y = src[0]
    assert np.array_equal(got[0], y)


def check_equal_sizes_nv21_is_a_swap_and_a_deinterleave(ctx, w, h):
    src, got = equal_size_call(ctx, "nv21", "nv12", w, h)
    assert np.array_equal(got[1], src[1][..., ::-1]), "NV21 -> NV12: the chroma plane with its bytes swapped"
    src, got = equal_size_call(ctx, "nv21", "y420p", w, h)
    assert np.array_equal(got[1], src[1][..., 1]) and np.array_equal(got[2], src[1][..., 0]), "NV21 -> y420p: Cb is byte 1, Cr byte 0"


def check_equal_sizes_422_chroma_columns_are_preserved(ctx, sfmt, dfmt):
    """a 4:2:2 chroma image is untouched horizontally (6 taps at 1:1: the centre weight 1, the others 0) and reduced 2:1 vertically.  With
    every chroma COLUMN constant — a seeded value per column — an output sample is fma-chained sum(w) * value of its own column; the twelve
    float weights sum to 1 within 1e-6, so the result is within 255e-6 of the integer value and rounds to it: every output row IS the source
    row, and a single horizontal tap that leaked from a neighbouring column would show"""
    w, h = 36, 20
    Y, Cb, Cr = D.logical(sfmt, D.alloc(sfmt, w, h, seed=77))
    Cb[:], Cr[:] = Cb[0], Cr[0]
    gs = D.to_gpu(ctx, sfmt, w, h, D.pack(sfmt, Y, Cb, Cr))
    gd = G.to_gpu(ctx, dfmt, w, h, util.alloc_image(dfmt, w, h, seed=5))
    sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420(c, gd, gs))
    gy, gcb, gcr = D.logical(dfmt, G.from_gpu(ctx, gd, dfmt, w, h))
    assert np.array_equal(gy, Y)
    assert gcb.shape == (h // 2, w // 2) and np.array_equal(gcb, np.broadcast_to(Cb[0], gcb.shape))
    assert np.array_equal(gcr, np.broadcast_to(Cr[0], gcr.shape))


# ---- 3. random geometries -------------------------------------------------------------------------------------------------------------
def random_geometry(seed, packed):
    rng = np.random.default_rng(9100 + seed)
    while True:
        ow, oh = int(rng.integers(2, 300)), int(rng.integers(2, 150))
        iw, ih = int(round(ow * float(rng.uniform(0.3, 6.0)))), int(round(oh * float(rng.uniform(0.3, 6.0))))
        if packed:
            iw &= ~1
        if 2 <= iw <= 600 and 2 <= ih <= 240 and 0.3 <= iw / ow <= 6.0 and 0.3 <= ih / oh <= 6.0:
            return iw, ih, ow, oh


def check_random_geometries(ctx, seed):
    """output sizes >= 2, per-axis picture ratio in [0.3, 6], even source width for packed formats: every draw must succeed"""
    sfmt, dfmt = D.FORMATS[seed % 5], D.TARGETS[(seed // 5) % 2]
    iw, ih, ow, oh = random_geometry(seed, sfmt in D.PACKED)
    assert not D.refused(sfmt, dfmt, iw, ih, ow, oh)
    run_single(ctx, sfmt, dfmt, iw, ih, ow, oh, seed=seed + 1)


# ---- 4. foreign layouts ----------------------------------------------------------------------------------------------------------------
def check_foreign_layouts(ctx, sfmt, dfmt, iw, ih, ow, oh, src_layout):
    src, exp = D.case(sfmt, dfmt, iw, ih, ow, oh, iw * 7 + oh)
    sources, placing = D.Sources(ctx), Placing(ctx)
    gs = sources.place(sfmt, iw, ih, src, src_layout)
    for dst_layout in ("guarded", "skewed", "at1p3"):
        gd = placing.place(dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=11), dst_layout)
        sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420(c, gd, gs))
        G.assert_same(placing.from_gpu(gd, dfmt, ow, oh), exp, f"{sfmt} -> {dfmt} {iw}x{ih} -> {ow}x{oh}, source on {src_layout}, target on {dst_layout}")
    sources.unchanged()
    placing.rec.sweep(ctx)          # every target allocation downloaded completely: its payload changed, nothing else


# ---- 5. ladders ------------------------------------------------------------------------------------------------------------------------
SRC = (96, 48)
STRIP = [(80, 40), (63, 31), (96, 48)]
MIXED = [(48, 24), (20, 10), (64, 32)]          # the middle one: more than 22 taps for every source, the tile route


def references(sfmt, dfmt, src_size, sizes, n):
    iw, ih = src_size
    srcs, exps = [None] * n, [[None] * n for _ in sizes]
    for r, (w, h) in enumerate(sizes):
        for i in range(n):
            srcs[i], exps[r][i] = D.case(sfmt, dfmt, iw, ih, w, h, 900 + i)
    return srcs, exps


def routes(sfmt, dfmt, src_size, sizes):
    return len({D.strip_route(sfmt, dfmt, *src_size, w, h) for w, h in sizes})


def check_three_rungs_of_five_pictures_equal_fifteen_single_calls(ctx, sfmt, dfmt, name, sizes):
    assert routes(sfmt, dfmt, SRC, sizes) == (2 if name == "mixed" else 1)
    srcs, exps = references(sfmt, dfmt, SRC, sizes, 5)
    gs = [D.to_gpu(ctx, sfmt, *SRC, s) for s in srcs]
    rungs, singles = fresh_targets(ctx, dfmt, sizes, 5, 3), fresh_targets(ctx, dfmt, sizes, 5, 1003)
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420Ladder(c, rungs, gs))
    assert counter() - before == routes(sfmt, dfmt, SRC, sizes), "one launch per route"
    for r in range(len(sizes)):
        for i in range(5):
            sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420(c, singles[r][i], gs[i]))
    check_rungs(ctx, dfmt, sizes, rungs, exps, f"{name} ladder {sfmt} -> {dfmt}", singles)


def check_eight_rungs_and_a_list_longer_than_one_chunk(ctx, sfmt, dfmt):
    """two chunks; the last rung takes the tile route: two launches per chunk, all rungs of a picture in one chunk"""
    src_size = (40, 24)
    sizes = [(40, 24), (56, 30), (36, 20), (30, 18), (27, 15), (24, 14), (20, 12), (6, 4)]
    assert routes(sfmt, dfmt, src_size, sizes) == 2 and not D.strip_route(sfmt, dfmt, *src_size, 6, 4)
    n = header_chunk(8, NP[dfmt], D.SRC_PLANES[sfmt]) + 1
    assert 2 < n < 20
    srcs, exps = references(sfmt, dfmt, src_size, sizes, n)
    gs = [D.to_gpu(ctx, sfmt, *src_size, s) for s in srcs]
    rungs = fresh_targets(ctx, dfmt, sizes, n, 7)
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420Ladder(c, rungs, gs))
    assert counter() - before == 4
    check_rungs(ctx, dfmt, sizes, rungs, exps, f"{n} pictures, eight rungs, {sfmt} -> {dfmt}")
    one = fresh_targets(ctx, dfmt, sizes, 1, 70)                                  # eight rungs of ONE picture
    sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420Ladder(c, one, gs[:1]))
    check_rungs(ctx, dfmt, sizes, one, [e[:1] for e in exps], f"one picture, eight rungs, {sfmt} -> {dfmt}")


def check_one_rung_of_n_equals_n_single_calls(ctx, sfmt, dfmt):
    sizes, n = [(63, 31)], 4
    srcs, exps = references(sfmt, dfmt, SRC, sizes, n)
    gs = [D.to_gpu(ctx, sfmt, *SRC, s) for s in srcs]
    rungs, singles = fresh_targets(ctx, dfmt, sizes, n, 9), fresh_targets(ctx, dfmt, sizes, n, 1009)
    ladder = sv.LanczosTo420Ladder(rungs, gs)
    sv.usingContext(ctx, lambda c: ladder.run(c))
    for i in range(n):
        sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420(c, singles[0][i], gs[i]))
    check_rungs(ctx, dfmt, sizes, rungs, exps, f"one rung of {n}, {sfmt} -> {dfmt}", singles)


def check_empty_ladders_are_noops(ctx):
    before = counter()
    lib = cv.load()
    cv.check(lib.chv_scale_lanczos_to_420_ladder(ctx.handle, None, 0, None, 3))
    cv.check(lib.chv_scale_lanczos_to_420_ladder(ctx.handle, None, 3, None, 0))
    assert sv.scaleLanczosTo420Ladder(ctx, [], []) is ctx
    assert counter() == before


# ---- 6. NV12 and y420p sources are forwarded ------------------------------------------------------------------------------------------------
def check_nv12_and_y420p_sources_equal_scale_lanczos_420(ctx, sfmt, dfmt):
    iw, ih, ow, oh = 36, 20, 24, 14
    gs = G.to_gpu(ctx, sfmt, iw, ih, util.alloc_image(sfmt, iw, ih, seed=12))
    a, b, l = (G.to_gpu(ctx, dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=s)) for s in (3, 4, 5))
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420(c, a, gs))
    sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420Ladder(c, [[l]], [gs]))
    assert counter() == before, "forwarded: this entry's launcher launched nothing"
    sv.usingContext(ctx, lambda c: sv.scaleLanczos420(c, b, gs))
    want = G.from_gpu(ctx, b, dfmt, ow, oh)
    G.assert_same(G.from_gpu(ctx, a, dfmt, ow, oh), want, f"{sfmt} -> {dfmt} through chv_scale_lanczos_to_420")
    G.assert_same(G.from_gpu(ctx, l, dfmt, ow, oh), want, f"{sfmt} -> {dfmt} through chv_scale_lanczos_to_420_ladder")


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------
class Decoded:
    """seeded sources of the five formats, kept alive: a descriptor borrows its picture's device memory"""

    def __init__(self, ctx):
        self.ctx, self.seed, self.made = ctx, 300, []

    def __call__(self, fmt, w, h):
        self.seed += 1
        self.made.append(D.to_gpu(self.ctx, fmt, w, h, D.alloc(fmt, w, h, self.seed)))
        return self.made[-1]


def single(ctx, d, s):
    return _case_of(cv.load().chv_scale_lanczos_to_420(ctx.handle, C.byref(d), C.byref(s)))


def ladder(ctx, rung_descs, src_descs):
    flat = [d for rung in rung_descs for d in rung]
    d, s = (cv.Image * len(flat))(*flat), (cv.Image * len(src_descs))(*src_descs)
    return _case_of(cv.load().chv_scale_lanczos_to_420_ladder(ctx.handle, d, len(rung_descs), s, len(src_descs)))


def chroma_only_refusal():
    """(iw, ih, ow, oh): a 4:4:4 picture whose luma reduction the 160 KB rule accepts and whose chroma reduction — twice as hard on both axes —
    it refuses, while the same picture as NV21 passes and a target twice as large passes as 4:4:4 too: found with the rule, the smallest first"""
    ow, oh = 16, 8
    for ky in range(4, 20):
        for kx in range(8, 30):
            iw, ih = ow * kx, oh * ky
            if not D.refuses(iw, ih, ow, oh) and D.refused("y444p", "nv12", iw, ih, ow, oh) and not D.refused("nv21", "nv12", iw, ih, ow, oh) \
                    and not D.refused("y444p", "nv12", iw, ih, 2 * ow, 2 * oh) and D.taps(iw, ow // 2) <= 256 and D.taps(ih, oh // 2) <= 256:
                return iw, ih, ow, oh
    raise AssertionError("no such geometry")


def check_errors_leave_every_target_unchanged(ctx):
    pic, dec, desc = Pictures(ctx), Decoded(ctx), sv._image_desc
    nv_d, yp_d, bg_d, bg_s = pic("nv12", 32, 18), pic("y420p", 32, 18), pic("bgra", 32, 18), pic("bgra", 64, 36)
    srcs = {f: dec(f, 64, 36) for f in D.FORMATS}
    # BAD_TARGET, as chv_scale_lanczos_420
    assert single(ctx, desc(bg_d), desc(srcs["nv21"])) == "badTarget"
    assert ladder(ctx, [[desc(bg_d)]], [desc(srcs["yuvs"])]) == "badTarget"
    bad = desc(yp_d)
    bad.planes[2].width -= 1
    assert single(ctx, bad, desc(srcs["y444p"])) == "badTarget"
    # BAD_INPUT: BGRA / RGBA; wrong plane or component counts; a plane that fails a plane check; Cb and Cr of different size; odd packed width
    assert single(ctx, desc(yp_d), desc(bg_s)) == "badInputData"
    assert ladder(ctx, [[desc(nv_d)]], [desc(bg_s)]) == "badInputData"
    bad = desc(srcs["y422p"]); bad.n_planes = 2
    assert single(ctx, desc(nv_d), bad) == "badInputData"
    bad = desc(srcs["yuvs"]); bad.planes[0].components = 1
    assert single(ctx, desc(nv_d), bad) == "badInputData"
    bad = desc(srcs["nv21"]); bad.planes[1].components = 1
    assert single(ctx, desc(yp_d), bad) == "badInputData"
    bad = desc(srcs["zvuy"]); bad.planes[0].offset = bad.planes[0].offset + (1 << 30)
    assert single(ctx, desc(yp_d), bad) == "badInputData"
    bad = desc(srcs["nv21"]); bad.planes[1].pitch = 3
    assert single(ctx, desc(yp_d), bad) == "badInputData"
    for skew in ("width", "height"):
        bad = desc(srcs["y444p"])
        setattr(bad.planes[1], skew, getattr(bad.planes[1], skew) - 1)
        assert single(ctx, desc(nv_d), bad) == "badInputData"
    for f in D.PACKED:
        bad = desc(srcs[f]); bad.planes[0].width = 63
        assert single(ctx, desc(nv_d), bad) == "badInputData"
    # INVALID_VALUE: the list's mistakes, bad counts, the 160 KB rule on ANY logical image
    two = [desc(srcs["y422p"]), desc(dec("y422p", 64, 36))]
    yp2 = pic("y420p", 32, 18)
    assert ladder(ctx, [[desc(yp_d), desc(nv_d)]], two) == "invalidValue"                                        # mixed target formats
    assert ladder(ctx, [[desc(yp_d), desc(yp2)]], [desc(srcs["y422p"]), desc(srcs["y444p"])]) == "invalidValue"   # mixed source formats
    assert ladder(ctx, [[desc(yp_d), desc(yp2)]], [desc(srcs["y422p"]), desc(dec("y422p", 62, 36))]) == "invalidValue"     # two source sizes
    assert ladder(ctx, [[desc(yp_d), desc(pic("y420p", 30, 18))]], two) == "invalidValue"                         # two sizes inside a rung
    nine = [[desc(pic("y420p", 8 + 2 * r, 6))] for r in range(9)]
    assert ladder(ctx, nine, [desc(srcs["nv21"])]) == "invalidValue"
    for counts in ((-1, 1), (1, -1)):
        assert _case_of(cv.load().chv_scale_lanczos_to_420_ladder(ctx.handle, C.byref(desc(nv_d)), counts[0], C.byref(desc(srcs["nv21"])), counts[1])) == "invalidValue"
    assert _case_of(cv.load().chv_scale_lanczos_to_420_ladder(ctx.handle, None, 1, C.byref(desc(srcs["nv21"])), 1)) == "invalidValue"
    iw, ih, ow, oh = chroma_only_refusal()
    wide444, wide_nv21, small, first = dec("y444p", iw, ih), dec("nv21", iw, ih), pic("nv12", ow, oh), pic("nv12", 2 * ow, 2 * oh)
    assert not D.refuses(iw, ih, ow, oh) and D.refused("y444p", "nv12", iw, ih, ow, oh) and not D.refused("nv21", "nv12", iw, ih, ow, oh)
    assert single(ctx, desc(small), desc(wide444)) == "invalidValue"              # luma passes, the 4:4:4 chroma does not
    assert ladder(ctx, [[desc(first)], [desc(small)]], [desc(wide444)]) == "invalidValue"      # refused in the LAST rung
    pic.unchanged("errors")
    # (the pictures the refusals were made from make good calls: every refusal above is the one it names)
    assert single(ctx, desc(small), desc(wide_nv21)) == "success"
    assert ladder(ctx, [[desc(first)]], [desc(wide444)]) == "success"
    for f in D.FORMATS:
        assert single(ctx, desc(nv_d), desc(srcs[f])) == "success" and single(ctx, desc(yp_d), desc(srcs[f])) == "success"


# ---- 8. inside a pass ------------------------------------------------------------------------------------------------------------------
def check_resize_inside_a_pass_sees_the_held_composite(ctx):
    """there is no composite kernel for the five formats: the NV12 canvas composited in the pass is handed to the resize described as NV21 —
    the same planes with Cb and Cr exchanged"""
    cw, ch, ow, oh = 128, 72, 64, 36
    layer = util.alloc_image("bgra", 40, 30, seed=7)
    u = util.make_uniforms((cw, ch), rect=(10, 6, 60, 40), border=(2, 2, 2, 2), fill=(0.2, 0.6, 0.3, 0.7), opacity=0.8, in_size=(40, 30))
    canvas = util.alloc_image("nv12", cw, ch, seed=8)
    assert O.run_kernel("img_clear_nv12", canvas) == 0
    assert O.run_kernel("img_bgra_nv12", canvas, layer, u) == 0
    (tw, th), (uw, uh) = D.logical_sizes("nv12", ow, oh)
    Y, Cb, Cr = D.logical("nv21", canvas)
    exp = D.pack("y420p", D.resize(Y, tw, th), D.resize(Cb, uw, uh), D.resize(Cr, uw, uh))
    gl = G.to_gpu(ctx, "bgra", 40, 30, layer)
    gc = G.to_gpu(ctx, "nv12", cw, ch, util.alloc_image("nv12", cw, ch, seed=8))
    as_nv21 = sv.PictureSample(gc.imageBuffer().withChanges(pixelFormat=sv.PixelFormat.nv21, planes=sv.decoderFramePlanes(sv.PixelFormat.nv21, (cw, ch)), buffers=[]))
    gd = G.to_gpu(ctx, "y420p", ow, oh, util.alloc_image("y420p", ow, oh, seed=9))

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gc, kernel=K("img_clear_nv12"), blends=False)
        c = sv.runComputeKernel(c, images=[gl], target=gc, kernel=K("img_bgra_nv12"), uniforms=u, blends=True)
        c = sv.scaleLanczosTo420(c, gd, as_nv21)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gc, "nv12", cw, ch), canvas, "the composited canvas")
    G.assert_same(G.from_gpu(ctx, gd, "y420p", ow, oh), exp, "the y420p rendition of the canvas composited in the same pass")


# ---- 9. PictureFilter ------------------------------------------------------------------------------------------------------------------
def check_picture_filter_flag_on_and_off(ctx, sfmt, dfmt):
    iw, ih, ow, oh = 96, 54, 64, 36
    src, exp = D.case(sfmt, dfmt, iw, ih, ow, oh, 41)
    f = sv.PictureFilter((ow, oh), G.FMT[dfmt], computeContext=ctx, scaler="lanczos", convertDecoderFormats=True)
    for sample in (sv.pictureFromDecoderFrame(D.fmt_of(sfmt), (iw, ih), src), D.to_gpu(ctx, sfmt, iw, ih, src)):
        kind, out = f(sample)
        assert kind == "just", out
        G.assert_same(G.from_gpu(f.context, out, dfmt, ow, oh), exp, f"PictureFilter lanczos {sfmt} -> {dfmt}")
    off = sv.PictureFilter((ow, oh), G.FMT[dfmt], computeContext=ctx, scaler="lanczos")
    kind, out = off(D.to_gpu(ctx, sfmt, iw, ih, src))
    assert kind == "error", "a host that did not ask for the conversion gets the error it got"


# ---- 10. upload and download carry decoder frames ------------------------------------------------------------------------------------------
def check_upload_and_download_carry_decoder_frames(ctx, sfmt):
    """planes as decoderFramePlanes describes them, strides from the frame's array (here: every row 5 bytes longer than its payload)"""
    w, h = 38, 18
    shapes = D.plane_shapes(sfmt, w, h)
    strides = [c * comps + 5 for _, c, comps in shapes]
    arrays = [util.splitmix_bytes(77 + k, r * s).reshape(r, s).copy() for k, ((r, _, _), s) in enumerate(zip(shapes, strides))]
    planes = sv.decoderFramePlanes(D.fmt_of(sfmt), (w, h), strides)
    assert [(p.size, p.stride, len(p.components)) for p in planes] == [((c, r), s, comps) for (r, c, comps), s in zip(shapes, strides)]
    with pytest.raises(sv.ComputeError):
        sv.planesForFormat(D.fmt_of(sfmt), (w, h))                   # (the reference's table does not know these formats, and keeps saying so)
    pict = sv.pictureFromDecoderFrame(D.fmt_of(sfmt), (w, h), arrays, strides)
    gpu = sv.uploadComputePicture(ctx, pict, retainCpuBuffer=False)
    back = sv.downloadComputePicture(ctx, gpu, retainGpuBuffer=True).imageBuffer().buffers
    for a, b, (r, c, comps) in zip(arrays, back, shapes):
        assert b.shape == a.shape and np.array_equal(b[:, : c * comps], a[:, : c * comps])
    # and the resize reads such a picture: the payload columns of the arrays are the picture
    src = [a[:, : c * comps] if comps == 1 else a[:, : c * comps].reshape(r, c, comps) for a, (r, c, comps) in zip(arrays, shapes)]
    (tw, th), (uw, uh) = D.logical_sizes("nv12", 21, 11)
    Y, Cb, Cr = D.logical(sfmt, [np.ascontiguousarray(p) for p in src])
    exp = D.pack("nv12", D.resize(Y, tw, th), D.resize(Cb, uw, uh), D.resize(Cr, uw, uh))
    gd = G.to_gpu(ctx, "nv12", 21, 11, util.alloc_image("nv12", 21, 11, seed=3))
    sv.usingContext(ctx, lambda c: sv.scaleLanczosTo420(c, gd, gpu))
    G.assert_same(G.from_gpu(ctx, gd, "nv12", 21, 11), exp, f"{sfmt} -> nv12 from an uploaded frame with padded rows")


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def cases():
    """(name, check, arguments) of every case, in the order of the sections above"""
    out = []

    def add(check, *args):
        out.append((check.__name__[6:] + "[" + "-".join("%dx%d" % tuple(a) if isinstance(a, tuple) and len(a) == 2 else str(a) for a in args) + "]", check, args))
    for p in shape_cells():
        add(check_named_shapes, *p.values)
    for w, h in [(34, 18), (130, 20), (2, 2)]:
        for s, d in CELLS:
            add(check_equal_sizes_luma_is_the_sources, s, d, w, h)
    for w, h in [(34, 18), (130, 20), (7, 5), (2, 2)]:
        add(check_equal_sizes_nv21_is_a_swap_and_a_deinterleave, w, h)
    for d in D.TARGETS:
        for s in ["y422p", "yuvs", "zvuy"]:
            add(check_equal_sizes_422_chroma_columns_are_preserved, s, d)
    for seed in range(32):
        add(check_random_geometries, seed)
    for layout in D.SOURCE_LAYOUTS:
        for shape in [(64, 20, 40, 14), (38, 18, 21, 11)]:       # (the first: rows of whole vectors in every format)
            for s, d in CELLS:
                add(check_foreign_layouts, s, d, *shape, layout)
    for name, sizes in [("strip", STRIP), ("mixed", MIXED)]:
        for s, d in CELLS:
            add(check_three_rungs_of_five_pictures_equal_fifteen_single_calls, s, d, name, sizes)
    for s, d in CELLS:
        add(check_eight_rungs_and_a_list_longer_than_one_chunk, s, d)
    for s, d in CELLS:
        add(check_one_rung_of_n_equals_n_single_calls, s, d)
    add(check_empty_ladders_are_noops)
    for d in D.TARGETS:
        for s in D.TARGETS:
            add(check_nv12_and_y420p_sources_equal_scale_lanczos_420, s, d)
    add(check_errors_leave_every_target_unchanged)
    add(check_resize_inside_a_pass_sees_the_held_composite)
    for s, d in CELLS:
        add(check_picture_filter_flag_on_and_off, s, d)
    for s in D.FORMATS:
        add(check_upload_and_download_carry_decoder_frames, s)
    add(check_cpp_mirror)
    return out


def check_cpp_mirror(ctx):
    """tests/cpp/test_lanczos_to_420.cpp: the C++ host mirror against the single calls (tests/test_cpp_lanczos_to_420.py builds it)"""
    import test_cpp_lanczos_to_420 as cpp
    cpp.run()


def test_every_case_is_in_the_table():
    """CPU: the table holds what the sections promise — 5 sources x 2 targets wherever a section says so, no name twice"""
    table = cases()
    names = [n for n, _, _ in table]
    assert len(set(names)) == len(names) and len(table) >= 320
    count = lambda check: sum(1 for _, c, _ in table if c is check)
    assert count(check_named_shapes) == 9 * 10 - 4 and count(check_random_geometries) == 32
    assert count(check_foreign_layouts) == 2 * len(D.SOURCE_LAYOUTS) * 10 and count(check_equal_sizes_luma_is_the_sources) == 30
    for check in (check_eight_rungs_and_a_list_longer_than_one_chunk, check_one_rung_of_n_equals_n_single_calls, check_picture_filter_flag_on_and_off):
        assert count(check) == 10
    assert count(check_three_rungs_of_five_pictures_equal_fifteen_single_calls) == 20
    checks = {v for k, v in globals().items() if k.startswith("check_") and callable(v)} - {check_rungs}
    assert checks == {c for _, c, _ in table}, "a check that no case runs"


@pytest.mark.gpu
def test_chv_scale_lanczos_to_420(ctx):
    failed = []
    for name, check, args in cases():
        try:
            check(ctx, *args)
        except AssertionError as e:
            failed.append(f"{name}: {str(e)[:600]}")
    assert not failed, "%d case(s) failed:\n%s" % (len(failed), "\n".join(failed[:20]))
