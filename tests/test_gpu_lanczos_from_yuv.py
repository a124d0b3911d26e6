"""chv_scale_lanczos_from_yuv / chv_scale_lanczos_from_yuv_batch: Lanczos-3 from an NV12 or y420p picture into a BGRA
or RGBA plane.  Bit-exact, no tolerance, no case excluded.

The expectation is built here from pieces that already exist.  The oracle's 4-channel Lanczos, whose channels are independent, gives the CODES
of the three logical planes at the target's size: Y replicated into all four channels in one call, Cb and Cr in channels 0 and 1 of a cw x ch
plane in another (how tests/test_gpu_lanczos_yuv.py pins a 1-component plane).  Then section 4.2 in numpy int64, from the table written out
below, spot-checked against the oracle's own matrix.  Every target is pre-filled with seeded bytes and whole planes are compared.  (The
one status of the entry that needs another BUILD — CHV_ERR_NOT_IMPLEMENTED without the kernel unit — is tests/test_lanczos_from_yuv_sanitizers.py's.)"""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest

import gpuutil as G
import layouts as L
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv
from test_gpu_lanczos_yuv import Placing

pytestmark = pytest.mark.gpu

K = sv.defaultComputeKernelFromString
SOURCES = ["nv12", "y420p"]
TARGETS = ["bgra", "rgba"]
KINDS = ["random", "primaries"]

# yoff, cy, crv, cgu, cgv, cbu
CSC = {0: (16, 76309, 104597, 25675, 53279, 132201),      # BT.601 limited
       1: (16, 76309, 117489, 13975, 34925, 138438),      # BT.709 limited
       2: (0, 65536, 91881, 22553, 46802, 116130),        # BT.601 full
       3: (0, 65536, 103206, 12276, 30679, 121609)}       # BT.709 full


def matrix(csc, y, u, v):
    """section 4.2 on arrays of codes -> (R, G, B) uint8"""
    yoff, cy, crv, cgu, cgv, cbu = CSC[csc]
    y, u, v = (np.asarray(a, dtype=np.int64) for a in (y, u, v))
    c = cy * (y - yoff) + 32768
    d, e = u - 128, v - 128
    clip8 = lambda a: np.clip(a >> 16, 0, 255).astype(np.uint8)        # noqa: E731
    return clip8(c + crv * e), clip8(c - cgu * d - cgv * e), clip8(c + cbu * d)


def test_the_matrix_written_out_here_is_the_oracles():
    rng = np.random.default_rng(42)
    corners = [(y, u, v) for y in (0, 255) for u in (0, 255) for v in (0, 255)]
    triples = np.array(corners + [(16, 128, 128), (235, 128, 128), (235, 240, 240), (16, 16, 16)] + rng.integers(0, 256, (300, 3)).tolist())
    for csc in range(4):
        r, g, b = matrix(csc, triples[:, 0], triples[:, 1], triples[:, 2])
        for i, (y, u, v) in enumerate(triples.tolist()):
            assert (int(r[i]), int(g[i]), int(b[i])) == O.yuv2rgb_int(csc, y, u, v), (csc, y, u, v)


def chroma_size(w, h):
    return max(1, w // 2), max(1, h // 2)


def codes(y, cb, cr, ow, oh):
    """the three logical planes resampled to ow x oh as chv_scale_lanczos resamples a 1-component plane"""
    ih, iw = y.shape
    ch, cw = cb.shape
    s4 = np.zeros((ih, iw, 4), dtype=np.uint8)
    s4[...] = y[..., None]
    d4 = np.zeros((oh, ow, 4), dtype=np.uint8)
    assert O.lanczos_bgra(d4, s4, threads=4) == 0, f"oracle refused luma {iw}x{ih} -> {ow}x{oh}"
    assert np.array_equal(d4[..., 0], d4[..., 3])
    c4 = np.zeros((ch, cw, 4), dtype=np.uint8)
    c4[..., 0], c4[..., 1] = cb, cr
    e4 = np.zeros((oh, ow, 4), dtype=np.uint8)
    assert O.lanczos_bgra(e4, c4, threads=4) == 0, f"oracle refused chroma {cw}x{ch} -> {ow}x{oh}"
    return d4[..., 0].copy(), e4[..., 0].copy(), e4[..., 1].copy()


def logical(fmt, planes):
    if fmt == "nv12":
        return np.asarray(planes[0]), np.asarray(planes[1])[..., 0], np.asarray(planes[1])[..., 1]
    return tuple(np.asarray(p) for p in planes)


def packed(fmt, y, cb, cr):
    """(Y, Cb, Cr) as the planes of a picture of packing `fmt`, shaped like util.alloc_image's"""
    if fmt == "nv12":
        return [y.copy(), np.ascontiguousarray(np.stack([cb, cr], axis=-1))]
    return [y.copy(), cb.copy(), cr.copy()]


def pixels(dfmt, csc, yc, uc, vc):
    r, g, b = matrix(csc, yc, uc, vc)
    a = np.full_like(r, 255)
    return [np.ascontiguousarray(np.stack([b, g, r, a] if dfmt == "bgra" else [r, g, b, a], axis=-1))]


def expected(sfmt, planes, ow, oh, dfmt, csc):
    return pixels(dfmt, csc, *codes(*logical(sfmt, planes), ow, oh))


def blocks(rng, h, w, values):
    """flat 8 x 8 blocks of seeded picks from `values`"""
    picks = rng.choice(np.array(values, dtype=np.uint8), size=((h + 7) // 8, (w + 7) // 8))
    return np.ascontiguousarray(np.kron(picks, np.ones((8, 8), dtype=np.uint8))[:h, :w])


@functools.lru_cache(maxsize=None)
def case(iw, ih, ow, oh, kind):
    """((Y, Cb, Cr) of the source, their codes at ow x oh) of one seeded case: computed once, shared (and left unchanged) by every test that
    names it — both packings, both target orders and all colourspaces start from these"""
    cw, ch = chroma_size(iw, ih)
    seed = iw * 7 + oh
    if kind == "random":
        y, cb, cr = (util.splitmix_bytes(seed * 16 + k, r * c).reshape(r, c).copy() for k, (r, c) in enumerate([(ih, iw), (ch, cw), (ch, cw)]))
    else:
        rng = np.random.default_rng(seed)
        y, cb, cr = blocks(rng, ih, iw, (0, 255, 16, 235)), blocks(rng, ch, cw, (0, 255, 16, 240)), blocks(rng, ch, cw, (0, 255, 16, 240))
    src = (y, cb, cr)
    for a in src:
        a.setflags(write=False)
    return src, codes(y, cb, cr, ow, oh)


def counter():
    return cv.get_counter("lanczos_from_yuv_launches")


def source_to_gpu(ctx, fmt, w, h, planes):
    """G.to_gpu; a 1-wide or 1-high picture is described by hand: the host's picture type rounds its chroma planes down to nothing, the C ABI
    (and this entry) take them as max(1, w // 2) x max(1, h // 2)"""
    if w >= 2 and h >= 2:
        return G.to_gpu(ctx, fmt, w, h, planes)
    desc, bufs = sv.planesForFormat(G.FMT[fmt], (w, h)), []
    for p, a in zip(desc, planes):
        p.size = (max(p.size[0], 1), max(p.size[1], 1))
        bufs.append(np.ascontiguousarray(a, dtype=np.uint8).reshape(p.size[1], -1))
        p.stride = bufs[-1].shape[1]
    return sv.uploadComputePicture(ctx, sv.PictureSample(sv.ImageBuffer(G.FMT[fmt], "cpu", (w, h), buffers=bufs, planes=desc)))


def run_single(ctx, sfmt, dfmt, iw, ih, ow, oh, kind, csc):
    src, cod = case(iw, ih, ow, oh, kind)
    gs = source_to_gpu(ctx, sfmt, iw, ih, packed(sfmt, *src))
    gd = G.to_gpu(ctx, dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=iw + 7))       # the target pre-filled with seeded bytes
    sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuv(c, gd, gs, colorspace=csc))
    G.assert_same(G.from_gpu(ctx, gd, dfmt, ow, oh), pixels(dfmt, csc, *cod), f"{sfmt} -> {dfmt} lanczos {iw}x{ih} -> {ow}x{oh}, {kind}, colourspace {csc}")


# ---- 1. named shapes ------------------------------------------------------------------------------------------------------------------
SHAPES = [(16, 16, 16, 16),          # equal size: luma codes pass through, chroma is enlarged 2x
          (36, 20, 24, 14),          # 10 luma taps, 6 chroma taps
          (256, 128, 128, 64),       # exact 2:1: chroma is 1:1
          (33, 17, 21, 11),          # odd source: cw = 16 against 33 luma columns
          (33, 17, 20, 10),          # tap counts differ between the axes
          (2, 2, 7, 5), (1, 1, 5, 3),                      # 1 x 1 chroma planes, enlargement
          (5, 3, 1, 1), (9, 7, 1, 4), (9, 7, 4, 1),        # degenerate targets
          (100, 50, 333, 171),       # several output rows per source row
          (440, 220, 200, 100),      # 14 luma taps, 8 chroma
          (700, 140, 200, 40),       # 22 luma taps, 12 chroma: the strip route's edge
          (64, 36, 17, 9),           # 24 taps: the tile route
          (600, 64, 50, 8),          # small tiles
          (1100, 40, 550, 20),       # several strips, the last one partial
          (1000, 202, 500, 101),     # several row chunks, odd last row
          (1920, 1080, 1280, 720)]   # one real size


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dfmt", TARGETS)
@pytest.mark.parametrize("sfmt", SOURCES)
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["%dx%d-%dx%d" % s for s in SHAPES])
def test_named_shapes(ctx, i, sfmt, dfmt, kind):
    """the colourspaces are spread over the cases; all four on the first shape"""
    spread = (i + SOURCES.index(sfmt) + 2 * TARGETS.index(dfmt) + KINDS.index(kind)) % 4
    for csc in (range(4) if i == 0 else [spread]):
        run_single(ctx, sfmt, dfmt, *SHAPES[i], kind, csc)


def test_null_opts_mean_bt601_limited(ctx):
    iw, ih, ow, oh = SHAPES[1]
    src, cod = case(iw, ih, ow, oh, "random")
    gs = G.to_gpu(ctx, "nv12", iw, ih, packed("nv12", *src))
    gd = G.to_gpu(ctx, "bgra", ow, oh, util.alloc_image("bgra", ow, oh, seed=3))
    d, s = sv._image_desc(gd), sv._image_desc(gs)
    cv.check(cv.load().chv_scale_lanczos_from_yuv(ctx.handle, C.byref(d), C.byref(s), None))
    G.assert_same(G.from_gpu(ctx, gd, "bgra", ow, oh), pixels("bgra", 0, *cod), "opts == NULL")


# ---- 2. batches ------------------------------------------------------------------------------------------------------------------------
def batch_case(sfmt, dfmt, iw, ih, ow, oh, n, csc):
    """n sources of one geometry that differ (picture i is the seeded case with i added to every byte), and what each must become"""
    (y, cb, cr), _ = case(iw, ih, ow, oh, "random")
    srcs = [packed(sfmt, y + np.uint8(i % 256), cb + np.uint8(3 * i % 256), cr + np.uint8(5 * i % 256)) for i in range(n)]      # (bytes wrap round)
    return srcs, [expected(sfmt, s, ow, oh, dfmt, csc) for s in srcs]


@pytest.mark.parametrize("dfmt", TARGETS)
@pytest.mark.parametrize("sfmt", SOURCES)
def test_batch_of_three_equals_single_calls(ctx, sfmt, dfmt):
    iw, ih, ow, oh, n, csc = 146, 40, 73, 20, 3, 1
    srcs, exps = batch_case(sfmt, dfmt, iw, ih, ow, oh, n, csc)
    gs = [G.to_gpu(ctx, sfmt, iw, ih, s) for s in srcs]
    gb, g1 = ([G.to_gpu(ctx, dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=seed + i)) for i in range(n)] for seed in (20, 40))
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuvBatch(c, list(zip(gb, gs)), colorspace=csc))
    assert counter() - before == 1
    for i in range(n):
        sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuv(c, g1[i], gs[i], colorspace=csc))
    assert counter() - before == 1 + n
    for i in range(n):
        got = G.from_gpu(ctx, gb[i], dfmt, ow, oh)
        G.assert_same(got, exps[i], f"batch of {n}, picture {i}, against the reference")
        G.assert_same(got, G.from_gpu(ctx, g1[i], dfmt, ow, oh), f"batch of {n}, picture {i}, against the single call")


@pytest.mark.parametrize("sfmt,chunk", [("nv12", 83), ("y420p", 62)])
def test_one_picture_more_than_a_chunk(ctx, sfmt, chunk):
    """a chunk is what fits one descriptor slot (the header states 83 / 62): chunk + 1 pictures leave in two launches"""
    header = (Path(__file__).resolve().parents[1] / "include" / "chipvideo.h").read_text()
    assert "83 pictures from NV12 (3 plane records each) or 62 from y420p (4 plane records each)" in header
    iw, ih, ow, oh, n, csc = 16, 16, 8, 8, chunk + 1, 2
    srcs, exps = batch_case(sfmt, "bgra", iw, ih, ow, oh, n, csc)
    gs = [G.to_gpu(ctx, sfmt, iw, ih, s) for s in srcs]
    gd = [G.to_gpu(ctx, "bgra", ow, oh, util.alloc_image("bgra", ow, oh, seed=60 + i)) for i in range(n)]
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuvBatch(c, list(zip(gd, gs)), colorspace=csc))
    assert counter() - before == 2
    for i in range(n):
        G.assert_same(G.from_gpu(ctx, gd[i], "bgra", ow, oh), exps[i], f"{n} {sfmt} pictures, picture {i}")


def test_an_empty_batch_is_a_noop(ctx):
    before = counter()
    cv.check(cv.load().chv_scale_lanczos_from_yuv_batch(ctx.handle, None, None, 0, None))
    assert sv.scaleLanczosFromYuvBatch(ctx, []) is ctx
    assert counter() == before


# ---- 3. errors -------------------------------------------------------------------------------------------------------------------------
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


def single(ctx, d, s, csc=0):
    opts = cv.KernelOpts(colorspace=csc)
    return _case_of(cv.load().chv_scale_lanczos_from_yuv(ctx.handle, C.byref(d), C.byref(s), C.byref(opts)))


def batch(ctx, ds, ss):
    d, s = (cv.Image * len(ds))(*ds), (cv.Image * len(ss))(*ss)
    return _case_of(cv.load().chv_scale_lanczos_from_yuv_batch(ctx.handle, d, s, len(ds), None))


def test_errors_leave_every_target_unchanged(ctx):
    pic, desc = Pictures(ctx), sv._image_desc
    nv_s, yp_s, bg_s = pic("nv12", 64, 36), pic("y420p", 64, 36), pic("bgra", 64, 36)
    bg_d, rg_d, nv_d, yp_d = pic("bgra", 32, 18), pic("rgba", 32, 18), pic("nv12", 32, 18), pic("y420p", 32, 18)
    before = counter()
    # the target: not one 4-component plane of format BGRA or RGBA, or a plane check
    assert single(ctx, desc(nv_d), desc(nv_s)) == "badTarget"
    assert single(ctx, desc(yp_d), desc(yp_s)) == "badTarget"
    bad = desc(bg_d)
    bad.format = cv.FMT_NV12
    assert single(ctx, bad, desc(nv_s)) == "badTarget"                          # one 4-component plane that calls itself NV12
    bad = desc(bg_d)
    bad.n_planes = 2
    assert single(ctx, bad, desc(nv_s)) == "badTarget"
    far = desc(bg_d)
    far.planes[0].height = 1 << 20                                              # a plane extent outside its buffer
    assert single(ctx, far, desc(nv_s)) == "badTarget"
    odd = desc(rg_d)
    odd.planes[0].pitch = odd.planes[0].pitch + 2                               # a 4-component plane must be 4-byte aligned
    odd.planes[0].height = 4
    assert single(ctx, odd, desc(yp_s)) == "badTarget"
    # the source: neither packing, unequal or wrong chroma planes, a plane check
    assert single(ctx, desc(bg_d), desc(bg_s)) == "badInputData"
    bad = desc(nv_s)
    bad.n_planes = 1
    assert single(ctx, desc(bg_d), bad) == "badInputData"
    bad = desc(yp_s)
    bad.format = cv.FMT_NV12                                                    # three planes that call themselves NV12
    assert single(ctx, desc(bg_d), bad) == "badInputData"
    for skew in ("width", "height"):
        bad = desc(yp_s)                                                        # a y420p picture with unequal chroma planes
        setattr(bad.planes[2], skew, getattr(bad.planes[2], skew) - 1)
        assert single(ctx, desc(bg_d), bad) == "badInputData"
        bad = desc(yp_s)                                                        # equal, but not half the luma plane
        for p in (1, 2):
            setattr(bad.planes[p], skew, getattr(bad.planes[p], skew) - 1)
        assert single(ctx, desc(rg_d), bad) == "badInputData"
        bad = desc(nv_s)
        setattr(bad.planes[1], skew, getattr(bad.planes[1], skew) - 1)
        assert single(ctx, desc(bg_d), bad) == "badInputData"
    far = desc(yp_s)
    far.planes[1].offset = far.planes[1].offset + (1 << 30)
    assert single(ctx, desc(bg_d), far) == "badInputData"
    comps = desc(nv_s)
    comps.planes[1].components = 1
    assert single(ctx, desc(bg_d), comps) == "badInputData"
    # the 160 KB rule on a logical plane's own sizes: 24:1
    big, tiny = pic("nv12", 96, 96), pic("bgra", 4, 4)
    assert single(ctx, desc(tiny), desc(big)) == "invalidValue"
    assert batch(ctx, [desc(tiny)], [desc(big)]) == "invalidValue"
    # lists: one geometry, one source format, one target format — all or nothing
    bg2, nv2, yp2 = pic("bgra", 32, 18), pic("nv12", 64, 36), pic("y420p", 64, 36)
    assert batch(ctx, [desc(bg_d), desc(pic("bgra", 30, 18))], [desc(nv_s), desc(nv2)]) == "invalidValue"          # two target sizes
    assert batch(ctx, [desc(bg_d), desc(bg2)], [desc(nv_s), desc(pic("nv12", 66, 36))]) == "invalidValue"          # two source sizes
    assert batch(ctx, [desc(bg_d), desc(bg2)], [desc(nv_s), desc(yp2)]) == "invalidValue"                          # two source formats
    assert batch(ctx, [desc(bg_d), desc(rg_d)], [desc(nv_s), desc(nv2)]) == "invalidValue"                         # two target orders
    assert batch(ctx, [desc(bg_d), desc(nv_d)], [desc(nv_s), desc(nv2)]) == "invalidValue"
    assert batch(ctx, [desc(bg_d), desc(bg2)], [desc(nv_s), desc(bg_s)]) == "invalidValue"
    with pytest.raises(sv.ComputeError) as e:                                   # a NULL list with a non-zero count
        cv.check(cv.load().chv_scale_lanczos_from_yuv_batch(ctx.handle, None, None, 2, None))
    assert e.value.case == "invalidValue"
    # every other entry keeps its statuses: no conversion happens in chv_scale_lanczos
    d, s = desc(bg_d), desc(nv_s)
    assert _case_of(cv.load().chv_scale_lanczos(ctx.handle, C.byref(d), C.byref(s))) == "badInputData"
    assert counter() == before, "a refused call launched something"
    pic.unchanged("errors")
    # (the pictures the refusals were made from make good calls: every refusal above is the one it names)
    assert single(ctx, desc(bg_d), desc(nv_s)) == "success"
    assert single(ctx, desc(rg_d), desc(yp_s), csc=3) == "success"
    assert batch(ctx, [desc(bg_d), desc(bg2)], [desc(nv_s), desc(nv2)]) == "success"


# ---- 4. foreign layouts ----------------------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(36, 20, 24, 14), (256, 128, 128, 64), (64, 36, 17, 9), (100, 50, 333, 171)]
# source planes at odd byte offsets with odd pitches (skewed), as views of larger parents (view); targets at a 4-byte but not 16-byte offset with
# a pitch that is no multiple of 16 (skewed: 4 mod 16 and row + 4; at4p4, at12p8)
LAYOUT_PAIRS = [(l, l) for l in L.LAYOUTS] + [("skewed", "at4p4"), ("view", "at12p8"), ("guarded", "skewed")]


@pytest.fixture
def placing(ctx):
    p = Placing(ctx)
    yield p
    p.rec.sweep(ctx)            # every allocation downloaded completely: payload of the targets changed, nothing else, no byte of a source


@pytest.mark.parametrize("sfmt,dfmt", [("nv12", "bgra"), ("y420p", "rgba")])
@pytest.mark.parametrize("iw,ih,ow,oh", LAYOUT_SHAPES)
@pytest.mark.parametrize("src_layout,dst_layout", LAYOUT_PAIRS)
def test_foreign_layouts(ctx, placing, sfmt, dfmt, iw, ih, ow, oh, src_layout, dst_layout):
    src, cod = case(iw, ih, ow, oh, "random")
    gs = placing.place(sfmt, iw, ih, packed(sfmt, *src), src_layout)
    gd = placing.place(dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=11), dst_layout)
    if dst_layout in ("skewed", "at4p4", "at12p8"):
        p = placing.rec.placement(gd).planes[0]
        assert p.offset % 4 == 0 and p.offset % 16 != 0 and p.pitch % 16 != 0
    sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuv(c, gd, gs, colorspace=1))
    G.assert_same(placing.from_gpu(gd, dfmt, ow, oh), pixels(dfmt, 1, *cod), f"{sfmt} -> {dfmt} {iw}x{ih} -> {ow}x{oh}, {src_layout} -> {dst_layout}")


# ---- 5. inside a pass ------------------------------------------------------------------------------------------------------------------
def test_conversion_inside_a_pass_sees_the_held_composite(ctx):
    cw, ch, ow, oh = 128, 72, 64, 36
    layer = util.alloc_image("bgra", 40, 30, seed=7)
    u = util.make_uniforms((cw, ch), rect=(10, 6, 60, 40), border=(2, 2, 2, 2), fill=(0.2, 0.6, 0.3, 0.7), opacity=0.8, in_size=(40, 30))
    canvas = util.alloc_image("nv12", cw, ch, seed=8)
    assert O.run_kernel("img_clear_nv12", canvas) == 0
    assert O.run_kernel("img_bgra_nv12", canvas, layer, u) == 0
    exp = expected("nv12", canvas, ow, oh, "bgra", 0)
    gl = G.to_gpu(ctx, "bgra", 40, 30, layer)
    gc = G.to_gpu(ctx, "nv12", cw, ch, util.alloc_image("nv12", cw, ch, seed=8))
    gd = G.to_gpu(ctx, "bgra", ow, oh, util.alloc_image("bgra", ow, oh, seed=9))

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gc, kernel=K("img_clear_nv12"), blends=False)
        c = sv.runComputeKernel(c, images=[gl], target=gc, kernel=K("img_bgra_nv12"), uniforms=u, blends=True)
        c = sv.scaleLanczosFromYuv(c, gd, gc)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gc, "nv12", cw, ch), canvas, "the composited canvas")
    G.assert_same(G.from_gpu(ctx, gd, "bgra", ow, oh), exp, "the BGRA rendition of the canvas composited in the same pass")


# ---- 6. PictureFilter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfmt,dfmt", [("nv12", "bgra"), ("y420p", "rgba")])
def test_picture_filter_convert_to_rgb(ctx, sfmt, dfmt):
    iw, ih, ow, oh, csc = 96, 54, 64, 36, 1
    src = util.alloc_image(sfmt, iw, ih, seed=41)
    exp = expected(sfmt, src, ow, oh, dfmt, csc)
    gs = G.to_gpu(ctx, sfmt, iw, ih, src)
    gd = G.to_gpu(ctx, dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=2))
    sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuv(c, gd, gs, colorspace=csc))
    entry = G.from_gpu(ctx, gd, dfmt, ow, oh)
    G.assert_same(entry, exp, "the entry against the reference")
    f = sv.PictureFilter((ow, oh), G.FMT[dfmt], computeContext=ctx, scaler="lanczos", colorspace=csc, convertToRgb=True)
    for sample in (sv.pictureFromArrays(G.FMT[sfmt], (iw, ih), src), gs):
        kind, out = f(sample)
        assert kind == "just", out
        G.assert_same(G.from_gpu(f.context, out, dfmt, ow, oh), entry, f"PictureFilter lanczos {sfmt} -> {dfmt}")
    # without the flag: what it raised before
    kind, out = sv.PictureFilter((ow, oh), G.FMT[dfmt], computeContext=ctx, scaler="lanczos", colorspace=csc)(gs)
    assert kind == "error" and out[0] == "filter.pict" and out[1] == -2 and "lanczos: BGRA -> BGRA, nv12 -> nv12 or y420p -> y420p only" in out[2], out
