"""chv_scale_lanczos_to_yuv / chv_scale_lanczos_to_yuv_batch: Lanczos-3 resize of a BGRA or RGBA plane into an NV12
or y420p picture in one launch.  Bit-exact, no tolerance, no case excluded.

The reference is built here: the oracle's 4-channel Lanczos gives the codes L, section 4.4.2 follows in numpy integers — luma of every pixel,
chroma of the rounded 2 x 2 box mean of L with clamped coordinates — with the coefficient tables rebuilt from the BT.601 / BT.709 luma weights
in exact rational arithmetic (as tests/test_rgb_to_yuv_int.py rebuilds them) and spot-checked against the oracle's integer matrix."""
import ctypes as C
import functools
import zlib
from fractions import Fraction as F

import numpy as np
import pytest

import gpuutil as G
import layouts as L
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv

pytestmark = pytest.mark.gpu

FORMATS = ["nv12", "y420p"]
ORDERS = ["bgra", "rgba"]
K = sv.defaultComputeKernelFromString

KW = {0: (F(299, 1000), F(114, 1000), True), 1: (F(2126, 10000), F(722, 10000), True),
      2: (F(299, 1000), F(114, 1000), False), 3: (F(2126, 10000), F(722, 10000), False)}


@functools.lru_cache(maxsize=None)
def tables(csc):
    """round(K * 65536 * range scale), green adjusted so that the luma row sums to round(65536 * 219 / 255) (65536 full range) and
    the chroma rows to 0"""
    kr, kb, limited = KW[csc]
    kg = 1 - kr - kb
    ys, cs = (F(219, 255), F(224, 255)) if limited else (F(1), F(1))
    rnd = lambda x: int((x * 65536 + F(1, 2)).__floor__())      # noqa: E731
    y = [rnd(kr * ys), rnd(kg * ys), rnd(kb * ys)]
    u = [rnd(-kr / (2 * (1 - kb)) * cs), rnd(-kg / (2 * (1 - kb)) * cs), rnd(F(1, 2) * cs)]
    v = [rnd(F(1, 2) * cs), rnd(-kg / (2 * (1 - kr)) * cs), rnd(-kb / (2 * (1 - kr)) * cs)]
    y[1] += rnd(ys) - sum(y); u[1] -= sum(u); v[1] -= sum(v)
    return (16 if limited else 0), tuple(y), tuple(u), tuple(v)


def source(kind, iw, ih, seed):
    """one (ih, iw, 4) plane.  'random': seeded bytes (mid-grey after the filter); 'blocks': 8 x 8 blocks of the eight 0 / 255 primaries with
    random alpha — flat areas at the corners of the RGB cube, so that the matrix reaches its extremes and the clips"""
    if kind == "random":
        return util.alloc_image("bgra", iw, ih, seed=seed)[0]
    rng = np.random.default_rng(seed)
    by, bx = (ih + 7) // 8, (iw + 7) // 8
    prim = rng.integers(0, 8, (by, bx))
    first = min(8, prim.size)
    prim.reshape(-1)[:first] = rng.permutation(8)[:first]          # every primary at least once
    cell = np.stack([((prim >> k) & 1) * 255 for k in range(3)], axis=-1).astype(np.uint8)
    img = np.zeros((ih, iw, 4), dtype=np.uint8)
    img[..., :3] = np.repeat(np.repeat(cell, 8, axis=0), 8, axis=1)[:ih, :iw]
    img[..., 3] = rng.integers(0, 256, (ih, iw))
    return img


@functools.lru_cache(maxsize=None)
def lanczos_codes(kind, iw, ih, ow, oh, seed):
    """(source plane, L): the four codes chv_scale_lanczos writes — computed once per case, shared and left unchanged"""
    src = source(kind, iw, ih, seed)
    d4 = np.zeros((oh, ow, 4), dtype=np.uint8)
    assert O.lanczos_bgra(d4, src, threads=4) == 0, f"oracle refused {iw}x{ih} -> {ow}x{oh}"
    src.setflags(write=False); d4.setflags(write=False)
    return src, d4


def to_yuv(fmt, order, codes, csc):
    """section 4.4.2 on the codes L -> planes shaped like util.alloc_image's"""
    oh, ow = codes.shape[:2]
    ri, bi = (2, 0) if order == "bgra" else (0, 2)
    r, g, b = (codes[..., i].astype(np.int64) for i in (ri, 1, bi))
    yoff, ky, ku, kv = tables(csc)
    clip = lambda t: np.clip(t >> 16, 0, 255).astype(np.uint8)      # noqa: E731
    luma = clip(ky[0] * r + ky[1] * g + ky[2] * b + (yoff << 16) + 32768)
    cw, chh = max(1, ow // 2), max(1, oh // 2)
    x0, y0 = 2 * np.arange(cw), 2 * np.arange(chh)
    x1, y1 = np.minimum(x0 + 1, ow - 1), np.minimum(y0 + 1, oh - 1)
    box = lambda c: (c[np.ix_(y0, x0)] + c[np.ix_(y0, x1)] + c[np.ix_(y1, x0)] + c[np.ix_(y1, x1)] + 2) >> 2      # noqa: E731
    mr, mg, mb = box(r), box(g), box(b)
    cb = clip(ku[0] * mr + ku[1] * mg + ku[2] * mb + (128 << 16) + 32768)
    cr = clip(kv[0] * mr + kv[1] * mg + kv[2] * mb + (128 << 16) + 32768)
    return [luma, np.stack([cb, cr], axis=-1)] if fmt == "nv12" else [luma, cb, cr]


def expected(fmt, order, kind, iw, ih, ow, oh, seed, csc):
    src, codes = lanczos_codes(kind, iw, ih, ow, oh, seed)
    return src, to_yuv(fmt, order, codes, csc)


def target_to_gpu(ctx, fmt, w, h, planes):
    """G.to_gpu for a target that may be 1 wide or 1 high: the hosts' picture model states chroma planes as w // 2 x h // 2 (the reference's
    planes), the C ABI and section 4.4.2 as max(1, w // 2) x max(1, h // 2) — the planes of such a picture are described by hand"""
    pict = sv.pictureFromArrays(G.FMT[fmt], (w, h), planes)
    for p in pict.imageBuffer().planes[1:]:
        p.size = (max(1, p.size[0]), max(1, p.size[1]))
    return sv.uploadComputePicture(ctx, pict)


def run_single(ctx, fmt, order, iw, ih, ow, oh, seed, csc, kind="random"):
    src, exp = expected(fmt, order, kind, iw, ih, ow, oh, seed, csc)
    gs = G.to_gpu(ctx, order, iw, ih, [src])
    gd = target_to_gpu(ctx, fmt, ow, oh, util.alloc_image(fmt, ow, oh, seed=seed + 7))   # the target pre-filled with seeded bytes
    sv.usingContext(ctx, lambda c: sv.scaleLanczosToYuv(c, gd, gs, colorspace=csc))
    G.assert_same(G.from_gpu(ctx, gd, fmt, ow, oh), exp, f"{order} -> {fmt} lanczos {iw}x{ih} -> {ow}x{oh}, colourspace {csc}, {kind} source")
    return exp


def test_the_reference_matrix_is_the_oracles():
    rng = np.random.default_rng(11)
    for csc in range(4):
        yoff, ky, ku, kv = tables(csc)
        for r, g, b in [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)] + rng.integers(0, 256, (200, 3)).tolist():
            codes = np.array([[[b, g, r, 9]]], dtype=np.uint8)
            y, c = to_yuv("nv12", "bgra", codes, csc)
            assert (int(y[0, 0]), int(c[0, 0, 0]), int(c[0, 0, 1])) == O.rgb2yuv_int(csc, r, g, b), (csc, r, g, b)


# ---- 1. named shapes ------------------------------------------------------------------------------------------------------------------
FIRST = [(16, 16, 16, 16),           # 6 taps; the matrix and the quad alone
         (36, 20, 24, 14),           # 10 taps, strip
         (256, 128, 128, 64)]        # exact 2:1
OTHERS = [(33, 17, 21, 11),          # odd output: luma-only last column and row
          (33, 17, 20, 10),          # tap counts differ between the axes: the tile kernel
          (2, 2, 7, 5),              # enlargement
          (5, 3, 1, 1), (9, 7, 1, 4), (9, 7, 4, 1),      # clamped quads
          (100, 50, 333, 171),       # several output rows per source row
          (440, 220, 200, 100),      # 14 taps
          (700, 140, 200, 40),       # 22 taps
          (64, 36, 17, 9),           # 24 taps, past the strips
          (600, 64, 50, 8),          # small tiles
          (1100, 40, 550, 20),       # several strips, the last partial
          (1000, 202, 500, 101),     # several row chunks and an odd last row
          (1920, 1080, 1280, 720)]   # real size


@pytest.mark.parametrize("csc", [0, 1, 2, 3])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("iw,ih,ow,oh", FIRST)
def test_first_shapes_every_colourspace_and_order(ctx, fmt, order, iw, ih, ow, oh, csc):
    run_single(ctx, fmt, order, iw, ih, ow, oh, seed=iw * 7 + oh, csc=csc)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n,shape", list(enumerate(OTHERS)))
def test_named_shapes(ctx, fmt, n, shape):
    iw, ih, ow, oh = shape
    run_single(ctx, fmt, ORDERS[n % 2], iw, ih, ow, oh, seed=iw * 7 + oh, csc=n % 4)


def test_2160p_to_1080p(ctx):
    run_single(ctx, "nv12", "bgra", 3840, 2160, 1920, 1080, seed=2160, csc=1)


@pytest.mark.parametrize("csc", [0, 1, 2, 3])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("iw,ih,ow,oh", [(36, 20, 24, 14), (256, 128, 128, 64)])
def test_primaries_reach_the_extremes(ctx, fmt, iw, ih, ow, oh, csc):
    """blocks of the 0 / 255 primaries: the expected planes hold the matrix's extremes, so the saturation of the Lanczos codes and the clip of
    the matrix are exercised.  Limited range: luma 16 / 235, chroma 16 / 240.  Full range: luma 0 / 255; chroma 255 is the CLIPPED 256 of pure
    blue / red (32768 x 255 + (128 << 16) + 32768 = 256 << 16), and its minimum over codes 0 .. 255 is 1 (yellow / cyan: -32768 x 255 + (128
    << 16) + 32768 = 1 << 16) — no RGB code triple gives 0."""
    exp = run_single(ctx, fmt, ORDERS[csc % 2], iw, ih, ow, oh, seed=502, csc=csc, kind="blocks")
    lo, hi, clo, chi = (16, 235, 16, 240) if csc < 2 else (0, 255, 1, 255)
    chroma = np.concatenate([np.asarray(p).reshape(-1) for p in exp[1:]])
    assert exp[0].min() == lo and exp[0].max() == hi, (exp[0].min(), exp[0].max())
    assert chroma.min() == clo and chroma.max() == chi, (chroma.min(), chroma.max())


# ---- 2. random geometries -------------------------------------------------------------------------------------------------------------
def random_geometry(seed):
    """the draw of tests/test_gpu_lanczos_yuv.py::random_geometry"""
    rng = np.random.default_rng(7300 + seed)
    while True:
        ow, oh = int(rng.integers(2, 400)), int(rng.integers(2, 200))
        iw, ih = int(round(ow * float(rng.uniform(0.3, 6.0)))), int(round(oh * float(rng.uniform(0.3, 6.0))))
        if 2 <= iw <= 700 and 2 <= ih <= 260 and 0.3 <= iw / ow <= 6.0 and 0.3 <= ih / oh <= 6.0:
            return iw, ih, ow, oh


@pytest.mark.parametrize("seed", range(32))
def test_random_geometries(ctx, seed):
    iw, ih, ow, oh = random_geometry(seed)
    run_single(ctx, FORMATS[seed % 2], ORDERS[(seed >> 1) % 2], iw, ih, ow, oh, seed=seed + 1, csc=(seed >> 2) % 4)


# ---- 3. foreign layouts ----------------------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(36, 20, 24, 14), (33, 17, 21, 11), (256, 64, 224, 56)]


class Placing:
    def __init__(self, ctx):
        self.ctx, self.rec, self.n = ctx, L.Recorder(), 0

    def place(self, fmt, w, h, planes, layout):
        self.n += 1
        return L.place(self.ctx, fmt, w, h, planes, layout, seed=(zlib.crc32(layout.encode()) & 0xFFFF) * 4096 + self.n, recorder=self.rec)

    def from_gpu(self, sample, fmt, w, h):
        return L.from_gpu(self.rec, G.from_gpu, self.ctx, sample, fmt, w, h)


@pytest.fixture
def placing(ctx):
    p = Placing(ctx)
    yield p
    p.rec.sweep(ctx)            # every allocation downloaded completely: payload of the targets changed, nothing else, no byte of a source


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("iw,ih,ow,oh", LAYOUT_SHAPES)
@pytest.mark.parametrize("src_layout,dst_layout", [(l, l) for l in L.LAYOUTS] + [("guarded", "skewed"), ("skewed", "guarded"), ("view", "tight"),
                                                   ("guarded", "at1p3"), ("guarded", "at4p4"), ("tight", "at2p6")])
def test_foreign_layouts(ctx, placing, fmt, iw, ih, ow, oh, src_layout, dst_layout):
    src, exp = expected(fmt, "bgra", "random", iw, ih, ow, oh, iw * 7 + oh, 0)
    gs = placing.place("bgra", iw, ih, [src], src_layout)
    gd = placing.place(fmt, ow, oh, util.alloc_image(fmt, ow, oh, seed=11), dst_layout)
    sv.usingContext(ctx, lambda c: sv.scaleLanczosToYuv(c, gd, gs))
    G.assert_same(placing.from_gpu(gd, fmt, ow, oh), exp, f"bgra -> {fmt} lanczos {iw}x{ih} -> {ow}x{oh}, source on {src_layout}, target on {dst_layout}")


# ---- 4. batches ------------------------------------------------------------------------------------------------------------------------
CHUNK = {"nv12": 83, "y420p": 62}          # pictures per descriptor slot (include/chipvideo.h)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("iw,ih,ow,oh,n", [(96, 54, 48, 27, 1), (96, 54, 48, 27, 3), (40, 24, 20, 12, None),
                                         (64, 36, 17, 9, 3)])          # (the last one: the tile kernel reads its pictures from the descriptor list)
def test_batch_equals_the_single_calls_and_the_reference(ctx, fmt, iw, ih, ow, oh, n):
    n = n or CHUNK[fmt] + 1
    order, csc = ("rgba", 3) if n == 3 else ("bgra", 0)
    pairs, singles, exps = [], [], []
    for i in range(n):
        src, exp = expected(fmt, order, "random", iw, ih, ow, oh, 900 + i, csc)
        exps.append(exp)
        gs = G.to_gpu(ctx, order, iw, ih, [src])
        pairs.append((G.to_gpu(ctx, fmt, ow, oh, util.alloc_image(fmt, ow, oh, seed=3 + i)), gs))
        singles.append((G.to_gpu(ctx, fmt, ow, oh, util.alloc_image(fmt, ow, oh, seed=5 + i)), gs))
    batch = sv.LanczosToYuvBatch(pairs, colorspace=csc)
    sv.usingContext(ctx, lambda c: batch.run(c))
    sv.usingContext(ctx, lambda c: batch.run(c))          # replayable
    for gd, gs in singles:
        sv.usingContext(ctx, lambda c: sv.scaleLanczosToYuv(c, gd, gs, colorspace=csc))
    for i, ((gd, _), (g1, _), exp) in enumerate(zip(pairs, singles, exps)):
        got = G.from_gpu(ctx, gd, fmt, ow, oh)
        G.assert_same(got, exp, f"batched {order} -> {fmt} lanczos, image {i} of {n}")
        G.assert_same(got, G.from_gpu(ctx, g1, fmt, ow, oh), f"batch against the single call, image {i} of {n}")


def test_empty_batch_is_a_noop(ctx):
    assert sv.LanczosToYuvBatch([]).run(ctx) is ctx
    cv.check(cv.load().chv_scale_lanczos_to_yuv_batch(ctx.handle, None, None, 0, None))


def _pair(ctx, fmt, order, iw, ih, ow, oh, seed):
    fill = util.alloc_image(fmt, ow, oh, seed=seed)
    return (G.to_gpu(ctx, fmt, ow, oh, fill), G.to_gpu(ctx, order, iw, ih, util.alloc_image(order, iw, ih, seed=seed + 1))), fill


def _rejected(ctx, pairs, fills, sizes):
    with pytest.raises(sv.ComputeError) as e:
        sv.LanczosToYuvBatch(pairs).run(ctx)
    assert e.value.case == "invalidValue", e.value
    for (gd, _), fill, (fmt, ow, oh) in zip(pairs, fills, sizes):
        G.assert_same(G.from_gpu(ctx, gd, fmt, ow, oh), fill, "a rejected batch wrote to a target")


def test_batch_rejects_mixed_target_formats(ctx):
    a, fa = _pair(ctx, "nv12", "bgra", 64, 36, 32, 18, 21)
    b, fb = _pair(ctx, "y420p", "bgra", 64, 36, 32, 18, 23)
    _rejected(ctx, [a, b], [fa, fb], [("nv12", 32, 18), ("y420p", 32, 18)])
    _rejected(ctx, [b, a], [fb, fa], [("y420p", 32, 18), ("nv12", 32, 18)])


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_rejects_mixed_source_formats(ctx, fmt):
    a, fa = _pair(ctx, fmt, "bgra", 64, 36, 32, 18, 25)
    b, fb = _pair(ctx, fmt, "rgba", 64, 36, 32, 18, 27)
    _rejected(ctx, [a, b], [fa, fb], [(fmt, 32, 18)] * 2)
    _rejected(ctx, [b, a], [fb, fa], [(fmt, 32, 18)] * 2)


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_rejects_mixed_geometry(ctx, fmt):
    a, fa = _pair(ctx, fmt, "bgra", 64, 36, 32, 18, 31)
    b, fb = _pair(ctx, fmt, "bgra", 80, 36, 32, 18, 33)
    c, fc = _pair(ctx, fmt, "bgra", 64, 36, 32, 20, 35)
    _rejected(ctx, [a, b], [fa, fb], [(fmt, 32, 18)] * 2)
    _rejected(ctx, [a, c], [fa, fc], [(fmt, 32, 18), (fmt, 32, 20)])


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------
def _status(ctx, d, s, batch=False):
    lib = cv.load()
    opts = cv.KernelOpts(colorspace=0)
    with pytest.raises(sv.ComputeError) as e:
        if batch:
            cv.check(lib.chv_scale_lanczos_to_yuv_batch(ctx.handle, C.byref(d), C.byref(s), 1, C.byref(opts)))
        else:
            cv.check(lib.chv_scale_lanczos_to_yuv(ctx.handle, C.byref(d), C.byref(s), C.byref(opts)))
    return e.value.case


@pytest.mark.parametrize("batch", [False, True])
def test_errors_leave_the_target_unchanged(ctx, batch):
    def picture(fmt, w, h, seed):
        planes = util.alloc_image(fmt, w, h, seed=seed)
        return G.to_gpu(ctx, fmt, w, h, planes), planes

    nv_s, _ = picture("nv12", 64, 36, 1)
    nv_d, nv_fill = picture("nv12", 32, 18, 2)
    yp_d, yp_fill = picture("y420p", 32, 18, 3)
    bg_d, bg_fill = picture("bgra", 32, 18, 4)
    bg_s, _ = picture("bgra", 64, 36, 5)
    big_s, _ = picture("bgra", 96, 96, 6)
    tiny_d, tiny_fill = picture("nv12", 4, 4, 7)
    desc = sv._image_desc
    st = lambda d, s: _status(ctx, d, s, batch)      # noqa: E731
    assert st(desc(bg_d), desc(bg_s)) == "badTarget"                            # a dst of BGRA
    one = desc(nv_d)
    one.n_planes = 1                                                            # an nv12 image with one plane
    assert st(one, desc(bg_s)) == "badTarget"
    three = desc(yp_d)
    three.format = cv.FMT_NV12                                                  # three planes that call themselves nv12
    assert st(three, desc(bg_s)) == "badTarget"
    far = desc(nv_d)                                                            # a chroma plane whose extent leaves its buffer
    far.planes[1].height = 1 << 20
    assert st(far, desc(bg_s)) == "badTarget"
    small = desc(yp_d)                                                          # a chroma plane that is not w / 2 x h / 2
    small.planes[2].width = 15
    assert st(small, desc(bg_s)) == "badTarget"
    assert st(desc(nv_d), desc(nv_s)) == "badInputData"                         # nv12 -> nv12 is chv_scale_lanczos's
    lie = desc(bg_s)
    lie.format = cv.FMT_NV12                                                    # one 4-component plane whose format says NV12
    assert st(desc(nv_d), lie) == "badInputData"
    far = desc(bg_s)
    far.planes[0].offset = far.planes[0].offset + (1 << 30)
    assert st(desc(yp_d), far) == "badInputData"
    odd = desc(bg_s)
    odd.planes[0].pitch = odd.planes[0].pitch + 2                               # a 4-component plane off its alignment
    assert st(desc(nv_d), odd) == "badInputData"
    assert st(desc(tiny_d), desc(big_s)) == "invalidValue"                      # 24:1: the 160 KB rule of chv_scale_lanczos
    bg_tiny, _ = picture("bgra", 4, 4, 8)
    with pytest.raises(sv.ComputeError) as e:                                   # (which refuses the same geometry)
        cv.check(cv.load().chv_scale_lanczos(ctx.handle, C.byref(desc(bg_tiny)), C.byref(desc(big_s))))
    assert e.value.case == "invalidValue"
    with pytest.raises(sv.ComputeError) as e:                                   # and chv_scale_lanczos keeps its answer for BGRA -> nv12
        cv.check(cv.load().chv_scale_lanczos(ctx.handle, C.byref(desc(nv_d)), C.byref(desc(bg_s))))
    assert e.value.case == "badInputData"
    for g, fmt, w, h, fill in ((nv_d, "nv12", 32, 18, nv_fill), (yp_d, "y420p", 32, 18, yp_fill), (bg_d, "bgra", 32, 18, bg_fill),
                               (tiny_d, "nv12", 4, 4, tiny_fill)):
        G.assert_same(G.from_gpu(ctx, g, fmt, w, h), fill, f"a refused call wrote to its {fmt} target")


def test_null_opts_mean_bt601_limited(ctx):
    iw, ih, ow, oh = 36, 20, 24, 14
    src, exp = expected("nv12", "bgra", "random", iw, ih, ow, oh, iw * 7 + oh, 0)
    gs = G.to_gpu(ctx, "bgra", iw, ih, [src])
    gd = G.to_gpu(ctx, "nv12", ow, oh, util.alloc_image("nv12", ow, oh, seed=1))
    d, s = sv._image_desc(gd), sv._image_desc(gs)
    cv.check(cv.load().chv_scale_lanczos_to_yuv(ctx.handle, C.byref(d), C.byref(s), None))
    G.assert_same(G.from_gpu(ctx, gd, "nv12", ow, oh), exp, "opts == NULL")


# ---- 6. inside a pass ------------------------------------------------------------------------------------------------------------------
def test_conversion_inside_a_pass_sees_the_held_composite(ctx):
    cw, ch, ow, oh = 128, 72, 64, 36
    layer = util.alloc_image("nv12", 40, 30, seed=7)
    u = util.make_uniforms((cw, ch), rect=(10, 6, 60, 40), border=(2, 2, 2, 2), fill=(0.2, 0.6, 0.3, 0.7), opacity=0.8, in_size=(40, 30))
    canvas = util.alloc_image("bgra", cw, ch, seed=8)
    assert O.run_kernel("img_clear_bgra", canvas) == 0
    assert O.run_kernel("img_nv12_bgra", canvas, layer, u) == 0
    d4 = np.zeros((oh, ow, 4), dtype=np.uint8)
    assert O.lanczos_bgra(d4, np.ascontiguousarray(canvas[0]), threads=4) == 0
    exp = to_yuv("nv12", "bgra", d4, 1)
    gl = G.to_gpu(ctx, "nv12", 40, 30, layer)
    gc = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=8))
    gd = G.to_gpu(ctx, "nv12", ow, oh, util.alloc_image("nv12", ow, oh, seed=9))

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gc, kernel=K("img_clear_bgra"), blends=False)
        c = sv.runComputeKernel(c, images=[gl], target=gc, kernel=K("img_nv12_bgra"), uniforms=u, blends=True)
        c = sv.scaleLanczosToYuv(c, gd, gc, colorspace=1)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gc, "bgra", cw, ch), canvas, "the composited canvas")
    G.assert_same(G.from_gpu(ctx, gd, "nv12", ow, oh), exp, "the rendition of the canvas composited in the same pass")


# ---- 7. PictureFilter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_picture_filter_lanczos_to_yuv(ctx, fmt, order):
    iw, ih, ow, oh = 96, 54, 64, 36
    src, exp = expected(fmt, order, "random", iw, ih, ow, oh, 41, 1)
    f = sv.PictureFilter((ow, oh), G.FMT[fmt], computeContext=ctx, scaler="lanczos", colorspace=cv.CSC_BT709_LIMITED)
    cpu = sv.pictureFromArrays(G.FMT[order], (iw, ih), [src])
    for sample in (cpu, G.to_gpu(ctx, order, iw, ih, [src])):
        kind, out = f(sample)
        assert kind == "just", out
        G.assert_same(G.from_gpu(f.context, out, fmt, ow, oh), exp, f"PictureFilter lanczos {order} -> {fmt}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_picture_filter_float_matrix_has_no_lanczos_form(ctx, fmt):
    f = sv.PictureFilter((64, 36), G.FMT[fmt], computeContext=ctx, scaler="lanczos", integerMatrix=False)
    kind, out = f(sv.pictureFromArrays(sv.PixelFormat.BGRA, (96, 54), util.alloc_image("bgra", 96, 54, seed=44)))
    assert kind == "error", out
