"""chv_scale_lanczos_hbd_to_420 / chv_scale_lanczos_hbd_to_420_ladder: Lanczos-3 from the two 10-bit 4:2:0 formats
(p010, y420p10) into NV12 and y420p pictures.  Bit-exact, no tolerance, no case excluded.

The cases are a TABLE run by one test (`cases()` at the end names them; the sections above are its checks): they share sources and
references, every case runs whether or not an earlier one failed, and the test reports each failed case by its name.  Anything but a failed
assertion — an error of the library or the runtime — ends the test at once.

The expected bytes are tests/hbd_formats.py's: every logical image (Y, Cb, Cr) of 10-bit codes through the restated chain on the oracle's
tables, the value divided by four before its one rounding, stored in the target's packing (tests/test_lanczos_hbd_reference.py pins that
reference on the CPU).  Every target is pre-filled with seeded bytes and whole planes are compared; every source carries seeded garbage in
the bits the format ignores."""
import ctypes as C

import numpy as np
import pytest

import gpuutil as G
import hbd_formats as H
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv
from test_gpu_lanczos_420 import Pictures, _case_of, check_rungs, fresh_targets, header_chunk
from test_gpu_lanczos_yuv import Placing

K = sv.defaultComputeKernelFromString
NP = {"nv12": 2, "y420p": 3}
CELLS = [(s, d) for s in H.FORMATS for d in H.TARGETS]


def counter():
    return cv.get_counter("lanczos_hbd_launches")


def run_single(ctx, sfmt, dfmt, iw, ih, ow, oh, seed, what=""):
    src, exp = H.case(sfmt, dfmt, iw, ih, ow, oh, seed)
    gs = H.to_gpu(ctx, sfmt, iw, ih, src)
    gd = G.to_gpu(ctx, dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=seed + 7))
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosHbdTo420(c, gd, gs))
    assert counter() - before == 1, "a single call takes one route: one launch"
    G.assert_same(G.from_gpu(ctx, gd, dfmt, ow, oh), exp, f"{sfmt} -> {dfmt} lanczos {iw}x{ih} -> {ow}x{oh} {what}")


# ---- 1. named shapes ------------------------------------------------------------------------------------------------------------------
# (iw, ih, ow, oh) -> (the strip body's tap class, None on the tile route)
SHAPES = {(2, 2, 2, 2): 6, (2, 2, 4, 4): 6,          # the smallest
          (34, 18, 34, 18): 6,                       # equal sizes
          (66, 34, 40, 22): 12,
          (20, 10, 66, 34): 6,                       # enlargement, a partial second strip
          (38, 18, 21, 11): 12, (33, 17, 21, 11): 12,          # odd targets: the last column and row own luma only
          (200, 12, 150, 8): 12,                     # three strips per row
          (130, 40, 40, 12): 22,                     # P010 -> y420p stages 60 of 64 vectors
          (96, 48, 20, 10): None,                    # 30 taps
          (40, 24, 6, 4): None}                      # 40 taps


def test_the_reference_accepts_every_named_shape_and_the_routes_are_the_expected_ones():
    """CPU only: the rules of tests/hbd_formats.py on the named shapes, before any of them runs"""
    for shape, T in SHAPES.items():
        for s, d in CELLS:
            assert not H.refused(s, d, *shape), (s, d, shape)
            assert H.strip_route(s, d, *shape) == (T is not None), (s, d, shape)
            if T is not None:
                assert H.tap_class(s, d, *shape)[1] == T, (s, d, shape)
    assert H.tap_class("p010", "nv12", 96, 48, 20, 10)[0] == 30 and H.tap_class("p010", "nv12", 40, 24, 6, 4)[0] == 40
    assert H.ring_vectors("p010", "y420p", 130, 40, 40, 12) == 60
    assert H.ring_vectors("y420p10", "nv12", 130, 40, 40, 12) == 36      # two chroma rows of 18 vectors in one ring slot


def check_named_shapes(ctx, sfmt, dfmt, iw, ih, ow, oh):
    run_single(ctx, sfmt, dfmt, iw, ih, ow, oh, seed=iw * 7 + oh)


# ---- 2. first principles at equal sizes: plain numpy, no reference ---------------------------------------------------------------------------
def every_code(w, h, seed):
    """(Y, Cb, Cr) that hold every code 0 .. 1023 at least once between them when the picture is large enough, each image when it has 1024 samples"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (iw, ih) in enumerate([(w, h), (max(w // 2, 1), max(h // 2, 1)), (max(w // 2, 1), max(h // 2, 1))]):
        n = iw * ih
        base = (np.arange(n) + 341 * k) % 1024 if n >= 342 else rng.integers(0, 1024, n)
        out.append(rng.permutation(base).astype(np.uint16).reshape(ih, iw))
    return out


def check_equal_sizes_every_byte_is_the_code_over_four(ctx, sfmt, dfmt, w, h):
    Y, Cb, Cr = every_code(w, h, w * 31 + h)
    if w * h >= 1024:
        assert len(set(Y.reshape(-1).tolist()) | set(Cb.reshape(-1).tolist()) | set(Cr.reshape(-1).tolist())) == 1024
    gs = H.to_gpu(ctx, sfmt, w, h, H.pack(sfmt, Y, Cb, Cr, seed=w + h))
    gd = G.to_gpu(ctx, dfmt, w, h, util.alloc_image(dfmt, w, h, seed=5))
    sv.usingContext(ctx, lambda c: sv.scaleLanczosHbdTo420(c, gd, gs))
    got = G.from_gpu(ctx, gd, dfmt, w, h)
    byte = lambda codes: np.minimum(np.rint(codes / 4.0), 255).astype(np.uint8)        # noqa: E731  (np.rint: ties to even)
    assert np.array_equal(got[0], byte(Y)), "Y"
    if dfmt == "nv12":
        assert np.array_equal(got[1], np.stack([byte(Cb), byte(Cr)], axis=-1)), "CbCr"
    else:
        assert np.array_equal(got[1], byte(Cb)) and np.array_equal(got[2], byte(Cr)), "Cb, Cr"


# ---- 3. random geometries -------------------------------------------------------------------------------------------------------------
def random_geometry(seed):
    rng = np.random.default_rng(9300 + seed)
    while True:
        ow, oh = int(rng.integers(2, 300)), int(rng.integers(2, 150))
        iw, ih = int(round(ow * float(rng.uniform(0.3, 6.0)))), int(round(oh * float(rng.uniform(0.3, 6.0))))
        if 2 <= iw <= 600 and 2 <= ih <= 240 and 0.3 <= iw / ow <= 6.0 and 0.3 <= ih / oh <= 6.0:
            return iw, ih, ow, oh


def check_random_geometries(ctx, seed):
    """output sizes >= 2, per-axis picture ratio in [0.3, 6]: every draw must be accepted"""
    sfmt, dfmt = CELLS[seed % 4]
    iw, ih, ow, oh = random_geometry(seed)
    assert not H.refused(sfmt, dfmt, iw, ih, ow, oh)
    run_single(ctx, sfmt, dfmt, iw, ih, ow, oh, seed=seed + 1)


# ---- 4. foreign layouts ----------------------------------------------------------------------------------------------------------------
def check_foreign_layouts(ctx, sfmt, dfmt, iw, ih, ow, oh, src_layout):
    src, exp = H.case(sfmt, dfmt, iw, ih, ow, oh, iw * 7 + oh)
    sources, placing = H.Sources(ctx), Placing(ctx)
    gs = sources.place(sfmt, iw, ih, src, src_layout)
    for dst_layout in ("guarded", "skewed", "at1p3"):
        gd = placing.place(dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=11), dst_layout)
        sv.usingContext(ctx, lambda c: sv.scaleLanczosHbdTo420(c, gd, gs))
        G.assert_same(placing.from_gpu(gd, dfmt, ow, oh), exp, f"{sfmt} -> {dfmt} {iw}x{ih} -> {ow}x{oh}, source on {src_layout}, target on {dst_layout}")
    sources.unchanged()
    placing.rec.sweep(ctx)          # every target allocation downloaded completely: its payload changed, nothing else


# ---- 5. ladders ------------------------------------------------------------------------------------------------------------------------
SRC = (96, 48)
STRIP = [(80, 40), (63, 31), (96, 48)]
MIXED = [(48, 24), (20, 10), (64, 32)]          # the middle one: 30 taps, the tile route


def references(sfmt, dfmt, src_size, sizes, n):
    iw, ih = src_size
    srcs, exps = [None] * n, [[None] * n for _ in sizes]
    for r, (w, h) in enumerate(sizes):
        for i in range(n):
            srcs[i], exps[r][i] = H.case(sfmt, dfmt, iw, ih, w, h, 900 + i)
    return srcs, exps


def routes(sfmt, dfmt, src_size, sizes):
    return len({H.strip_route(sfmt, dfmt, *src_size, w, h) for w, h in sizes})


def check_three_rungs_of_five_pictures_equal_fifteen_single_calls(ctx, sfmt, dfmt, name, sizes):
    assert routes(sfmt, dfmt, SRC, sizes) == (2 if name == "mixed" else 1)
    srcs, exps = references(sfmt, dfmt, SRC, sizes, 5)
    gs = [H.to_gpu(ctx, sfmt, *SRC, s) for s in srcs]
    rungs, singles = fresh_targets(ctx, dfmt, sizes, 5, 3), fresh_targets(ctx, dfmt, sizes, 5, 1003)
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosHbdTo420Ladder(c, rungs, gs))
    assert counter() - before == routes(sfmt, dfmt, SRC, sizes), "one launch per route"
    for r in range(len(sizes)):
        for i in range(5):
            sv.usingContext(ctx, lambda c: sv.scaleLanczosHbdTo420(c, singles[r][i], gs[i]))
    check_rungs(ctx, dfmt, sizes, rungs, exps, f"{name} ladder {sfmt} -> {dfmt}", singles)


def check_eight_rungs_and_a_list_longer_than_one_chunk(ctx, sfmt, dfmt):
    """two chunks; the last rung takes the tile route: two launches per chunk, all rungs of a picture in one chunk"""
    src_size = (40, 24)
    sizes = [(40, 24), (56, 30), (36, 20), (30, 18), (27, 15), (24, 14), (20, 12), (6, 4)]
    assert routes(sfmt, dfmt, src_size, sizes) == 2 and not H.strip_route(sfmt, dfmt, *src_size, 6, 4)
    n = header_chunk(8, NP[dfmt], H.SRC_PLANES[sfmt]) + 1
    assert 2 < n < 20
    srcs, exps = references(sfmt, dfmt, src_size, sizes, n)
    gs = [H.to_gpu(ctx, sfmt, *src_size, s) for s in srcs]
    rungs = fresh_targets(ctx, dfmt, sizes, n, 7)
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosHbdTo420Ladder(c, rungs, gs))
    assert counter() - before == 4
    check_rungs(ctx, dfmt, sizes, rungs, exps, f"{n} pictures, eight rungs, {sfmt} -> {dfmt}")


def check_one_rung_of_four_equals_four_single_calls(ctx, sfmt, dfmt):
    sizes, n = [(63, 31)], 4
    srcs, exps = references(sfmt, dfmt, SRC, sizes, n)
    gs = [H.to_gpu(ctx, sfmt, *SRC, s) for s in srcs]
    rungs, singles = fresh_targets(ctx, dfmt, sizes, n, 9), fresh_targets(ctx, dfmt, sizes, n, 1009)
    ladder_ = sv.LanczosHbdTo420Ladder(rungs, gs)
    sv.usingContext(ctx, lambda c: ladder_.run(c))
    for i in range(n):
        sv.usingContext(ctx, lambda c: sv.scaleLanczosHbdTo420(c, singles[0][i], gs[i]))
    check_rungs(ctx, dfmt, sizes, rungs, exps, f"one rung of {n}, {sfmt} -> {dfmt}", singles)


def check_empty_ladders_are_noops(ctx):
    before = counter()
    lib = cv.load()
    cv.check(lib.chv_scale_lanczos_hbd_to_420_ladder(ctx.handle, None, 0, None, 3))
    cv.check(lib.chv_scale_lanczos_hbd_to_420_ladder(ctx.handle, None, 3, None, 0))
    assert sv.scaleLanczosHbdTo420Ladder(ctx, [], []) is ctx
    assert counter() == before


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------
class Decoded:
    """seeded 10-bit sources, kept alive: a descriptor borrows its picture's device memory"""

    def __init__(self, ctx):
        self.ctx, self.seed, self.made = ctx, 300, []

    def __call__(self, fmt, w, h):
        self.seed += 1
        self.made.append(H.to_gpu(self.ctx, fmt, w, h, H.pack(fmt, *H.random_codes(w, h, self.seed), seed=self.seed)))
        return self.made[-1]


def single(ctx, d, s):
    return _case_of(cv.load().chv_scale_lanczos_hbd_to_420(ctx.handle, C.byref(d), C.byref(s)))


def ladder(ctx, rung_descs, src_descs):
    flat = [d for rung in rung_descs for d in rung]
    d, s = (cv.Image * len(flat))(*flat), (cv.Image * len(src_descs))(*src_descs)
    return _case_of(cv.load().chv_scale_lanczos_hbd_to_420_ladder(ctx.handle, d, len(rung_descs), s, len(src_descs)))


def refused_geometry():
    """(iw, ih, ow, oh): the smallest reduction of this family that the 160 KB rule refuses while a target twice as large passes"""
    ow, oh = 16, 8
    for ky in range(4, 40):
        for kx in range(8, 40):
            iw, ih = ow * kx, oh * ky
            if H.refused("p010", "nv12", iw, ih, ow, oh) and not H.refused("p010", "nv12", iw, ih, 2 * ow, 2 * oh) \
                    and H.taps(iw, ow // 2) <= 256 and H.taps(ih, oh // 2) <= 256:
                return iw, ih, ow, oh
    raise AssertionError("no such geometry")


def check_errors_leave_every_target_unchanged(ctx):
    pic, dec, desc = Pictures(ctx), Decoded(ctx), sv._image_desc
    nv_d, yp_d, bg_d = pic("nv12", 32, 18), pic("y420p", 32, 18), pic("bgra", 32, 18)
    srcs = {f: dec(f, 64, 36) for f in H.FORMATS}
    p010, y10 = srcs["p010"], srcs["y420p10"]
    # BAD_TARGET, as chv_scale_lanczos_420
    assert single(ctx, desc(bg_d), desc(p010)) == "badTarget"
    assert ladder(ctx, [[desc(bg_d)]], [desc(y10)]) == "badTarget"
    bad = desc(yp_d); bad.planes[2].width -= 1
    assert single(ctx, bad, desc(y10)) == "badTarget"
    # BAD_INPUT: 8-bit sources are not forwarded; wrong plane or component counts; a failed plane check; odd start, odd pitch; Cb != Cr
    for fmt in ("nv12", "y420p", "bgra"):
        assert single(ctx, desc(nv_d), desc(pic(fmt, 64, 36))) == "badInputData", fmt
    nv21 = sv.PictureSample(pic("nv12", 64, 36).imageBuffer().withChanges(pixelFormat=sv.PixelFormat.nv21, planes=sv.decoderFramePlanes(sv.PixelFormat.nv21, (64, 36)), buffers=[]))
    assert single(ctx, desc(yp_d), desc(nv21)) == "badInputData"
    assert ladder(ctx, [[desc(nv_d)]], [desc(pic("y420p", 64, 36))]) == "badInputData"
    bad = desc(y10); bad.n_planes = 2
    assert single(ctx, desc(nv_d), bad) == "badInputData"
    bad = desc(p010); bad.planes[0].components = 1
    assert single(ctx, desc(nv_d), bad) == "badInputData"
    bad = desc(p010); bad.planes[1].components = 2
    assert single(ctx, desc(yp_d), bad) == "badInputData"
    bad = desc(y10); bad.planes[0].offset = bad.planes[0].offset + (1 << 30)
    assert single(ctx, desc(yp_d), bad) == "badInputData"
    bad = desc(p010); bad.planes[1].pitch = 6
    assert single(ctx, desc(yp_d), bad) == "badInputData"
    for fmt, p in (("p010", 0), ("p010", 1), ("y420p10", 2)):
        bad = desc(srcs[fmt]); bad.planes[p].offset += 1; bad.planes[p].height -= 1
        assert single(ctx, desc(nv_d), bad) == "badInputData", f"odd start, {fmt} plane {p}"
        bad = desc(srcs[fmt]); bad.planes[p].pitch += 1; bad.planes[p].height = 2          # (two rows: the longer pitch stays inside the buffer)
        assert single(ctx, desc(nv_d), bad) == "badInputData", f"odd pitch, {fmt} plane {p}"
    for skew in ("width", "height"):
        bad = desc(y10)
        setattr(bad.planes[1], skew, getattr(bad.planes[1], skew) - 1)
        assert single(ctx, desc(nv_d), bad) == "badInputData"
    # INVALID_VALUE: the list's mistakes, bad counts, the 160 KB rule
    two = [desc(p010), desc(dec("p010", 64, 36))]
    yp2 = pic("y420p", 32, 18)
    assert ladder(ctx, [[desc(yp_d), desc(nv_d)]], two) == "invalidValue"                                        # mixed target formats
    assert ladder(ctx, [[desc(yp_d), desc(yp2)]], [desc(p010), desc(y10)]) == "invalidValue"                       # mixed source formats
    assert ladder(ctx, [[desc(yp_d), desc(yp2)]], [desc(p010), desc(dec("p010", 62, 36))]) == "invalidValue"       # two source sizes
    assert ladder(ctx, [[desc(yp_d), desc(pic("y420p", 30, 18))]], two) == "invalidValue"                         # two sizes inside a rung
    nine = [[desc(pic("y420p", 8 + 2 * r, 6))] for r in range(9)]
    assert ladder(ctx, nine, [desc(p010)]) == "invalidValue"
    for counts in ((-1, 1), (1, -1)):
        assert _case_of(cv.load().chv_scale_lanczos_hbd_to_420_ladder(ctx.handle, C.byref(desc(nv_d)), counts[0], C.byref(desc(p010)), counts[1])) == "invalidValue"
    assert _case_of(cv.load().chv_scale_lanczos_hbd_to_420_ladder(ctx.handle, None, 1, C.byref(desc(p010)), 1)) == "invalidValue"
    iw, ih, ow, oh = refused_geometry()
    wide, small, first = dec("p010", iw, ih), pic("nv12", ow, oh), pic("nv12", 2 * ow, 2 * oh)
    assert single(ctx, desc(small), desc(wide)) == "invalidValue"
    assert ladder(ctx, [[desc(first)], [desc(small)]], [desc(wide)]) == "invalidValue"      # refused in the LAST rung
    # the existing entries refuse the two new formats with the status they give any unknown format
    lib = cv.load()
    for s in (p010, y10):
        assert _case_of(lib.chv_scale_lanczos(ctx.handle, C.byref(desc(nv_d)), C.byref(desc(s)))) == "badInputData"
        assert _case_of(lib.chv_scale_lanczos_420(ctx.handle, C.byref(desc(nv_d)), C.byref(desc(s)))) == "badInputData"
        assert _case_of(lib.chv_scale_lanczos_to_420(ctx.handle, C.byref(desc(yp_d)), C.byref(desc(s)))) == "badInputData"
        assert _case_of(lib.chv_scale_lanczos_420_ladder(ctx.handle, C.byref(desc(yp_d)), 1, C.byref(desc(s)), 1)) == "badInputData"
        assert _case_of(lib.chv_scale_lanczos_to_420_ladder(ctx.handle, C.byref(desc(yp_d)), 1, C.byref(desc(s)), 1)) == "badInputData"
    pic.unchanged("errors")
    # (the pictures the refusals were made from make good calls: every refusal above is the one it names)
    assert ladder(ctx, [[desc(first)]], [desc(wide)]) == "success"
    for f in H.FORMATS:
        assert single(ctx, desc(nv_d), desc(srcs[f])) == "success" and single(ctx, desc(yp_d), desc(srcs[f])) == "success"
    assert ladder(ctx, [[desc(yp_d), desc(yp2)]], two) == "success"


# ---- 7. inside a pass ------------------------------------------------------------------------------------------------------------------
def check_resize_inside_a_pass_sees_the_held_composite(ctx):
    """there is no composite kernel for 10-bit canvases: the 128 x 72 y420p canvas composited in the pass is handed to the resize described as
    a 64 x 72 y420p10 picture — the same planes, two bytes to a word"""
    cw, ch, ow, oh = 128, 72, 40, 36
    layer = util.alloc_image("bgra", 40, 30, seed=7)
    u = util.make_uniforms((cw, ch), rect=(10, 6, 60, 40), border=(2, 2, 2, 2), fill=(0.2, 0.6, 0.3, 0.7), opacity=0.8, in_size=(40, 30))
    canvas = util.alloc_image("y420p", cw, ch, seed=8)
    assert O.run_kernel("img_clear_y420p", canvas) == 0
    assert O.run_kernel("img_bgra_y420p", canvas, layer, u) == 0
    words = [np.ascontiguousarray(p).view("<u2") for p in canvas]
    assert [w.shape for w in words] == [(72, 64), (36, 32), (36, 32)]
    exp = H.reference("y420p10", "nv12", words, ow, oh)
    gl = G.to_gpu(ctx, "bgra", 40, 30, layer)
    gc = G.to_gpu(ctx, "y420p", cw, ch, util.alloc_image("y420p", cw, ch, seed=8))
    as_10 = sv.PictureSample(gc.imageBuffer().withChanges(pixelFormat=sv.PixelFormat.y420p10, size=(cw // 2, ch),
                                                          planes=sv.decoderFramePlanes(sv.PixelFormat.y420p10, (cw // 2, ch)), buffers=[]))
    gd = G.to_gpu(ctx, "nv12", ow, oh, util.alloc_image("nv12", ow, oh, seed=9))

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gc, kernel=K("img_clear_y420p"), blends=False)
        c = sv.runComputeKernel(c, images=[gl], target=gc, kernel=K("img_bgra_y420p"), uniforms=u, blends=True)
        c = sv.scaleLanczosHbdTo420(c, gd, as_10)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gc, "y420p", cw, ch), canvas, "the composited canvas")
    G.assert_same(G.from_gpu(ctx, gd, "nv12", ow, oh), exp, "the NV12 rendition of the canvas composited in the same pass")


# ---- 8. PictureFilter ------------------------------------------------------------------------------------------------------------------
def check_picture_filter_flag_on_and_off(ctx, sfmt, dfmt):
    iw, ih, ow, oh = 96, 54, 64, 36
    src, exp = H.case(sfmt, dfmt, iw, ih, ow, oh, 41)
    f = sv.PictureFilter((ow, oh), G.FMT[dfmt], computeContext=ctx, scaler="lanczos", convertHighBitDepth=True)
    for sample in (sv.pictureFromDecoderFrame(H.fmt_of(sfmt), (iw, ih), H.as_bytes(src)), H.to_gpu(ctx, sfmt, iw, ih, src)):
        kind, out = f(sample)
        assert kind == "just", out
        G.assert_same(G.from_gpu(f.context, out, dfmt, ow, oh), exp, f"PictureFilter lanczos {sfmt} -> {dfmt}")
    for off in (sv.PictureFilter((ow, oh), G.FMT[dfmt], computeContext=ctx, scaler="lanczos"),
                sv.PictureFilter((ow, oh), G.FMT[dfmt], computeContext=ctx, scaler="lanczos", convertDecoderFormats=True)):
        kind, out = off(H.to_gpu(ctx, sfmt, iw, ih, src))
        assert kind == "error", "a host that did not ask for the conversion gets the error it got"


# ---- 9. upload and download carry 10-bit frames ----------------------------------------------------------------------------------------------
def check_upload_and_download_carry_frames_with_padded_rows(ctx, sfmt):
    """planes as decoderFramePlanes describes them, strides from the frame's array (here: every row 6 bytes longer than its payload)"""
    w, h = 38, 18
    shapes = H.plane_shapes(sfmt, w, h)
    strides = [c * comps + 6 for _, c, comps in shapes]
    arrays = [util.splitmix_bytes(77 + k, r * s).reshape(r, s).copy() for k, ((r, _, _), s) in enumerate(zip(shapes, strides))]
    planes = sv.decoderFramePlanes(H.fmt_of(sfmt), (w, h), strides)
    assert [(p.size, p.stride, len(p.components), p.bitDepth) for p in planes] == [((c, r), s, comps, 10) for (r, c, comps), s in zip(shapes, strides)]
    assert H.fmt_of(sfmt) in sv.HIGH_BIT_DEPTH_FORMATS and H.fmt_of(sfmt) not in sv.DECODER_FORMATS
    with pytest.raises(sv.ComputeError):
        sv.planesForFormat(H.fmt_of(sfmt), (w, h))                   # (the reference's table does not know these formats, and keeps saying so)
    pict = sv.pictureFromDecoderFrame(H.fmt_of(sfmt), (w, h), arrays, strides)
    gpu = sv.uploadComputePicture(ctx, pict, retainCpuBuffer=False)
    back = sv.downloadComputePicture(ctx, gpu, retainGpuBuffer=True).imageBuffer().buffers
    for a, b, (r, c, comps) in zip(arrays, back, shapes):
        assert b.shape == a.shape and np.array_equal(b[:, : c * comps], a[:, : c * comps])
    # and the resize reads such a picture: the payload columns of the arrays are the picture's words
    words = [np.ascontiguousarray(a[:, : c * comps]).view("<u2") for a, (r, c, comps) in zip(arrays, shapes)]
    if sfmt == "p010":
        words[1] = words[1].reshape(words[1].shape[0], -1, 2)
    exp = H.reference(sfmt, "nv12", words, 21, 11)
    gd = G.to_gpu(ctx, "nv12", 21, 11, util.alloc_image("nv12", 21, 11, seed=3))
    sv.usingContext(ctx, lambda c: sv.scaleLanczosHbdTo420(c, gd, gpu))
    G.assert_same(G.from_gpu(ctx, gd, "nv12", 21, 11), exp, f"{sfmt} -> nv12 from an uploaded frame with padded rows")


def check_cpp_mirror(ctx):
    """tests/cpp/test_lanczos_hbd.cpp: the C++ host mirror against the single calls (tests/test_cpp_lanczos_hbd.py builds it)"""
    import test_cpp_lanczos_hbd as cpp
    cpp.run()


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def cases():
    """(name, check, arguments) of every case, in the order of the sections above"""
    out = []

    def add(check, *args):
        out.append((check.__name__[6:] + "[" + "-".join("%dx%d" % tuple(a) if isinstance(a, tuple) and len(a) == 2 else str(a) for a in args) + "]", check, args))
    for shape in SHAPES:
        for s, d in CELLS:
            add(check_named_shapes, s, d, *shape)
    for w, h in [(34, 18), (130, 20), (7, 5), (2, 2)]:
        for s, d in CELLS:
            add(check_equal_sizes_every_byte_is_the_code_over_four, s, d, w, h)
    for seed in range(24):
        add(check_random_geometries, seed)
    for layout in H.SOURCE_LAYOUTS:
        for shape in [(64, 20, 40, 14), (38, 18, 21, 11)]:       # (the first: rows of whole vectors in every plane)
            for s, d in CELLS:
                add(check_foreign_layouts, s, d, *shape, layout)
    for name, sizes in [("strip", STRIP), ("mixed", MIXED)]:
        for s, d in CELLS:
            add(check_three_rungs_of_five_pictures_equal_fifteen_single_calls, s, d, name, sizes)
    for s, d in CELLS:
        add(check_eight_rungs_and_a_list_longer_than_one_chunk, s, d)
    for s, d in CELLS:
        add(check_one_rung_of_four_equals_four_single_calls, s, d)
    add(check_empty_ladders_are_noops)
    add(check_errors_leave_every_target_unchanged)
    add(check_resize_inside_a_pass_sees_the_held_composite)
    for s, d in CELLS:
        add(check_picture_filter_flag_on_and_off, s, d)
    for s in H.FORMATS:
        add(check_upload_and_download_carry_frames_with_padded_rows, s)
    add(check_cpp_mirror)
    return out


def test_every_case_is_in_the_table():
    """CPU: the table holds what the sections promise — 2 sources x 2 targets wherever a section says so, no name twice"""
    table = cases()
    names = [n for n, _, _ in table]
    assert len(set(names)) == len(names)
    count = lambda check: sum(1 for _, c, _ in table if c is check)        # noqa: E731
    assert count(check_named_shapes) == 11 * 4 and count(check_random_geometries) == 24
    assert count(check_foreign_layouts) == 2 * len(H.SOURCE_LAYOUTS) * 4 and count(check_equal_sizes_every_byte_is_the_code_over_four) == 16
    assert {CELLS[seed % 4] for seed in range(24)} == set(CELLS)
    for seed in range(24):
        assert not H.refused(*CELLS[seed % 4], *random_geometry(seed)), seed
    assert {H.strip_route(*CELLS[seed % 4], *random_geometry(seed)) for seed in range(24)} == {True, False}
    checks = {v for k, v in globals().items() if k.startswith("check_") and callable(v)} - {check_rungs}
    assert checks == {c for _, c, _ in table}, "a check that no case runs"


@pytest.mark.gpu
def test_chv_scale_lanczos_hbd_to_420(ctx):
    failed = []
    for name, check, args in cases():
        try:
            check(ctx, *args)
        except AssertionError as e:
            failed.append(f"{name}: {str(e)[:600]}")
    assert not failed, "%d case(s) failed:\n%s" % (len(failed), "\n".join(failed[:20]))
