"""chv_scale_lanczos / chv_scale_lanczos_batch on NV12 and y420p pictures: plane-wise Lanczos-3.

The reference is built here from the oracle's 4-channel Lanczos, whose channels are independent: a 1-component plane is replicated into all four
channels (any channel of the result is the plane's), the CbCr plane of NV12 goes into channels 0 and 1.  Every plane is resampled as an image of
its own — its own (in, out) tables per axis from its own width and height; chroma planes are max(1, w // 2) x max(1, h // 2)."""
import ctypes as C
import functools
import zlib

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
K = sv.defaultComputeKernelFromString


def plane_sizes(fmt, w, h):
    return [(max(c, 1), max(r, 1), comps) for r, c, comps in util.plane_shapes(fmt, w, h)]


def reference(fmt, src, iw, ih, ow, oh):
    """the plane-wise resize of `src` (util.alloc_image planes) through orc_lanczos_bgra -> planes shaped like util.alloc_image's"""
    out = []
    for plane, (pw, ph, comps), (qw, qh, _) in zip(src, plane_sizes(fmt, iw, ih), plane_sizes(fmt, ow, oh)):
        s4 = np.zeros((ph, pw, 4), dtype=np.uint8)
        if comps == 1:
            s4[...] = np.asarray(plane).reshape(ph, pw, 1)
        else:
            s4[..., :2] = np.asarray(plane).reshape(ph, pw, 2)
        d4 = np.zeros((qh, qw, 4), dtype=np.uint8)
        assert O.lanczos_bgra(d4, s4, threads=4) == 0, f"oracle refused plane {pw}x{ph} -> {qw}x{qh}"
        if comps == 1:
            assert np.array_equal(d4[..., 0], d4[..., 3])
            out.append(d4[..., 0].copy())
        else:
            out.append(d4[..., :2].copy())
    return out


@functools.lru_cache(maxsize=None)
def case(fmt, iw, ih, ow, oh, seed):
    """(source planes, expected planes) of one seeded case: computed once, shared (and left unchanged) by every test that names it"""
    src = util.alloc_image(fmt, iw, ih, seed=seed)
    return src, reference(fmt, src, iw, ih, ow, oh)


def run_single(ctx, fmt, iw, ih, ow, oh, seed, what=""):
    src, exp = case(fmt, iw, ih, ow, oh, seed)
    gs = G.to_gpu(ctx, fmt, iw, ih, src)
    gd = G.to_gpu(ctx, fmt, ow, oh, util.alloc_image(fmt, ow, oh, seed=seed + 7))        # the target pre-filled with seeded bytes
    sv.usingContext(ctx, lambda c: sv.scaleLanczos(c, gd, gs))
    G.assert_same(G.from_gpu(ctx, gd, fmt, ow, oh), exp, f"{fmt} lanczos {iw}x{ih} -> {ow}x{oh} {what}")


# ---- 1. named shapes ------------------------------------------------------------------------------------------------------------------
SHAPES = [(16, 16, 16, 16),          # 6 taps
          (36, 20, 24, 14),          # 3:2
          (256, 128, 128, 64),       # exact 2:1 on every plane
          (146, 20, 73, 10),         # 12 taps luma, 14 taps chroma
          (33, 17, 20, 10),          # odd sizes, floor'd chroma; tap counts differ between the axes of a plane
          (8, 8, 5, 5),              # chroma 4x4 -> 2x2: narrower than a vector
          (2, 2, 7, 5),              # 1x1 chroma enlarged
          (100, 50, 333, 171),       # enlargement: output rows sharing all their source rows
          (240, 120, 200, 100),      # 8 taps
          (440, 220, 200, 100),      # 14 taps
          (600, 300, 200, 100),      # 18 taps
          (700, 140, 200, 40),       # 22 taps: the widest staged row
          (64, 36, 17, 9),           # 24 taps: past the strip route
          (600, 64, 50, 8),          # 12:1 / 8:1
          (1100, 40, 550, 20),       # several strips per plane, the last one partial
          (1000, 200, 500, 100),     # several row chunks with a short tail
          (1920, 1080, 1280, 720)]   # one real size


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("iw,ih,ow,oh", SHAPES)
def test_named_shapes(ctx, fmt, iw, ih, ow, oh):
    run_single(ctx, fmt, iw, ih, ow, oh, seed=iw * 7 + oh)


# rows of whole 16-byte vectors at 4-byte addresses take the hand-awaited loads in every strip, the strips on the plane's edges included (a lane
# outside the row replicates the edge texel of the row's first / last vector): one shape per instantiation, reductions and an enlargement
VECTOR_ROW_SHAPES = [(64, 32, 200, 90),        # 6 taps, enlargement: the left and right edge vectors of every plane replicated
                     (256, 64, 224, 56),       # 8 taps
                     (512, 96, 352, 66),       # 10 taps in the 12-tap instantiation, several strips
                     (512, 256, 200, 100),     # 16 taps
                     (704, 144, 200, 40),      # 22 taps
                     (1280, 64, 640, 32)]      # exact 2:1, 10 luma strips


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("iw,ih,ow,oh", VECTOR_ROW_SHAPES)
def test_vector_row_shapes(ctx, fmt, iw, ih, ow, oh):
    run_single(ctx, fmt, iw, ih, ow, oh, seed=iw * 5 + oh)


# ---- 2. random geometries -------------------------------------------------------------------------------------------------------------
def random_geometry(seed):
    rng = np.random.default_rng(7300 + seed)
    while True:
        ow, oh = int(rng.integers(2, 400)), int(rng.integers(2, 200))
        iw, ih = int(round(ow * float(rng.uniform(0.3, 6.0)))), int(round(oh * float(rng.uniform(0.3, 6.0))))
        if 2 <= iw <= 700 and 2 <= ih <= 260 and 0.3 <= iw / ow <= 6.0 and 0.3 <= ih / oh <= 6.0:
            return iw, ih, ow, oh


@pytest.mark.parametrize("seed", range(32))
def test_random_geometries(ctx, seed):
    """output sizes >= 2, per-axis ratio in [0.3, 6]: every draw must succeed (the chroma ratio stays under 10:1)"""
    iw, ih, ow, oh = random_geometry(seed)
    run_single(ctx, FORMATS[seed % 2], iw, ih, ow, oh, seed=seed + 1)


# ---- 3. foreign layouts ----------------------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(36, 20, 24, 14), (146, 20, 73, 10), (8, 8, 5, 5), (1100, 40, 550, 20), (100, 50, 333, 171),
                 (256, 128, 128, 64)]          # (the last one: rows of whole vectors — the hand-awaited loads wherever the layout aligns them)


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
@pytest.mark.parametrize("src_layout,dst_layout", [(l, l) for l in L.LAYOUTS] + [("guarded", "at1p3"), ("guarded", "at4p4")])
def test_foreign_layouts(ctx, placing, fmt, iw, ih, ow, oh, src_layout, dst_layout):
    src, exp = case(fmt, iw, ih, ow, oh, iw * 7 + oh)
    gs = placing.place(fmt, iw, ih, src, src_layout)
    gd = placing.place(fmt, ow, oh, util.alloc_image(fmt, ow, oh, seed=11), dst_layout)
    sv.usingContext(ctx, lambda c: sv.scaleLanczos(c, gd, gs))
    G.assert_same(placing.from_gpu(gd, fmt, ow, oh), exp, f"{fmt} lanczos {iw}x{ih} -> {ow}x{oh}, source on {src_layout}, target on {dst_layout}")


# ---- 4. batches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("iw,ih,ow,oh,n", [(96, 54, 48, 27, 5), (200, 120, 75, 45, 70), (40, 24, 20, 12, 130),
                                         (64, 36, 17, 9, 3)])          # (the last one: 24 taps — the tile kernel reads its pictures from the descriptor list)
def test_batch_equals_the_reference_image_by_image(ctx, fmt, iw, ih, ow, oh, n):
    pairs, exps = [], []
    for i in range(n):
        src, exp = case(fmt, iw, ih, ow, oh, 900 + i)
        exps.append(exp)
        pairs.append((G.to_gpu(ctx, fmt, ow, oh, util.alloc_image(fmt, ow, oh, seed=3 + i)), G.to_gpu(ctx, fmt, iw, ih, src)))
    batch = sv.LanczosBatch(pairs)
    sv.usingContext(ctx, lambda c: batch.run(c))
    sv.usingContext(ctx, lambda c: batch.run(c))          # replayable
    for i, ((gd, _), exp) in enumerate(zip(pairs, exps)):
        G.assert_same(G.from_gpu(ctx, gd, fmt, ow, oh), exp, f"batched {fmt} lanczos, image {i} of {n}")


def test_empty_batch_is_a_noop(ctx):
    assert sv.LanczosBatch([]).run(ctx) is ctx


def _pair(ctx, fmt, iw, ih, ow, oh, seed):
    fill = util.alloc_image(fmt, ow, oh, seed=seed)
    return (G.to_gpu(ctx, fmt, ow, oh, fill), G.to_gpu(ctx, fmt, iw, ih, util.alloc_image(fmt, iw, ih, seed=seed + 1))), fill


def _rejected(ctx, pairs, fills, sizes):
    with pytest.raises(sv.ComputeError) as e:
        sv.LanczosBatch(pairs).run(ctx)
    assert e.value.case == "invalidValue", e.value
    for (gd, _), fill, (fmt, ow, oh) in zip(pairs, fills, sizes):
        G.assert_same(G.from_gpu(ctx, gd, fmt, ow, oh), fill, "a rejected batch wrote to a target")


def test_batch_rejects_mixed_formats(ctx):
    a, fa = _pair(ctx, "nv12", 64, 36, 32, 18, 21)
    b, fb = _pair(ctx, "y420p", 64, 36, 32, 18, 23)
    _rejected(ctx, [a, b], [fa, fb], [("nv12", 32, 18), ("y420p", 32, 18)])
    _rejected(ctx, [b, a], [fb, fa], [("y420p", 32, 18), ("nv12", 32, 18)])


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_that_begins_with_bgra_rejects_a_420_picture(ctx, fmt):
    a, fa = _pair(ctx, "bgra", 64, 36, 32, 18, 25)
    b, fb = _pair(ctx, fmt, 64, 36, 32, 18, 27)
    _rejected(ctx, [a, b], [fa, fb], [("bgra", 32, 18), (fmt, 32, 18)])


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_rejects_mixed_geometry(ctx, fmt):
    a, fa = _pair(ctx, fmt, 64, 36, 32, 18, 31)
    b, fb = _pair(ctx, fmt, 80, 36, 32, 18, 33)
    c, fc = _pair(ctx, fmt, 64, 36, 32, 20, 35)
    _rejected(ctx, [a, b], [fa, fb], [(fmt, 32, 18)] * 2)
    _rejected(ctx, [a, c], [fa, fc], [(fmt, 32, 18), (fmt, 32, 20)])


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------
def _status(ctx, d, s):
    lib = cv.load()
    with pytest.raises(sv.ComputeError) as e:
        cv.check(lib.chv_scale_lanczos(ctx.handle, C.byref(d), C.byref(s)))
    return e.value.case


def test_errors_leave_the_target_unchanged(ctx):
    def picture(fmt, w, h, seed):
        planes = util.alloc_image(fmt, w, h, seed=seed)
        return G.to_gpu(ctx, fmt, w, h, planes), planes

    nv_s, _ = picture("nv12", 64, 36, 1)
    nv_d, nv_fill = picture("nv12", 32, 18, 2)
    yp_d, yp_fill = picture("y420p", 32, 18, 3)
    bg_d, bg_fill = picture("bgra", 32, 18, 4)
    bg_s, _ = picture("bgra", 64, 36, 5)
    desc = sv._image_desc
    assert _status(ctx, desc(yp_d), desc(nv_s)) == "badInputData"               # nv12 -> y420p
    assert _status(ctx, desc(bg_d), desc(nv_s)) == "badInputData"               # nv12 -> BGRA
    assert _status(ctx, desc(nv_d), desc(bg_s)) == "badInputData"               # BGRA -> nv12
    one = desc(nv_d)
    one.n_planes = 1                                                            # an nv12 image with one plane
    assert _status(ctx, one, desc(nv_s)) == "badTarget"
    one = desc(nv_s)
    one.n_planes = 1
    assert _status(ctx, desc(nv_d), one) == "badInputData"
    far = desc(nv_d)                                                            # a chroma plane whose extent leaves its buffer
    far.planes[1].height = 1 << 20
    assert _status(ctx, far, desc(nv_s)) == "badTarget"
    far = desc(nv_s)
    far.planes[1].offset = far.planes[1].offset + (1 << 30)
    assert _status(ctx, desc(nv_d), far) == "badInputData"
    for g, fmt, fill in ((nv_d, "nv12", nv_fill), (yp_d, "y420p", yp_fill), (bg_d, "bgra", bg_fill)):
        G.assert_same(G.from_gpu(ctx, g, fmt, 32, 18), fill, f"a refused call wrote to its {fmt} target")


# ---- 6. table cache --------------------------------------------------------------------------------------------------------------------
def test_table_cache_eviction_keeps_results_exact(ctx):
    """70 nv12 target sizes from one source, four tables each: more than the cache's 64 entries, past one retire batch"""
    iw, ih = 96, 40
    sizes = [(20 + 2 * i, 10 + 2 * (i % 9)) for i in range(70)] + [(20, 10)]
    assert len(set(sizes)) == 70
    src = util.alloc_image("nv12", iw, ih, seed=77)
    gs = G.to_gpu(ctx, "nv12", iw, ih, src)
    for n, (ow, oh) in enumerate(sizes):
        gd = G.to_gpu(ctx, "nv12", ow, oh, util.alloc_image("nv12", ow, oh, seed=5))
        sv.usingContext(ctx, lambda c: sv.scaleLanczos(c, gd, gs))
        if n % 10 == 0 or n == len(sizes) - 1:
            G.assert_same(G.from_gpu(ctx, gd, "nv12", ow, oh), reference("nv12", src, iw, ih, ow, oh), f"nv12 lanczos {iw}x{ih} -> {ow}x{oh}, call {n}")


# ---- 7. PictureFilter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_picture_filter_lanczos(ctx, fmt):
    iw, ih, ow, oh = 96, 54, 64, 36
    src, exp = case(fmt, iw, ih, ow, oh, 41)
    f = sv.PictureFilter((ow, oh), G.FMT[fmt], computeContext=ctx, scaler="lanczos")
    cpu = sv.pictureFromArrays(G.FMT[fmt], (iw, ih), src)
    for sample in (cpu, G.to_gpu(ctx, fmt, iw, ih, src)):
        kind, out = f(sample)
        assert kind == "just", out
        G.assert_same(G.from_gpu(f.context, out, fmt, ow, oh), exp, f"PictureFilter lanczos {fmt}")


def test_picture_filter_lanczos_keeps_refusing_conversions(ctx):
    src = util.alloc_image("nv12", 96, 54, seed=42)
    f = sv.PictureFilter((64, 36), sv.PixelFormat.BGRA, computeContext=ctx, scaler="lanczos")
    kind, out = f(sv.pictureFromArrays(sv.PixelFormat.nv12, (96, 54), src))
    assert kind == "error", out
    f = sv.PictureFilter((64, 36), sv.PixelFormat.nv12, computeContext=ctx, scaler="lanczos")
    kind, out = f(sv.pictureFromArrays(sv.PixelFormat.y420p, (96, 54), util.alloc_image("y420p", 96, 54, seed=43)))
    assert kind == "error", out


# ---- 8. inside a pass ------------------------------------------------------------------------------------------------------------------
def test_resize_inside_a_pass_sees_the_held_composite(ctx):
    cw, ch, ow, oh = 128, 72, 64, 36
    layer = util.alloc_image("bgra", 40, 30, seed=7)
    u = util.make_uniforms((cw, ch), rect=(10, 6, 60, 40), border=(2, 2, 2, 2), fill=(0.2, 0.6, 0.3, 0.7), opacity=0.8, in_size=(40, 30))
    canvas = util.alloc_image("nv12", cw, ch, seed=8)
    assert O.run_kernel("img_clear_nv12", canvas) == 0
    assert O.run_kernel("img_bgra_nv12", canvas, layer, u) == 0
    exp = reference("nv12", canvas, cw, ch, ow, oh)
    gl = G.to_gpu(ctx, "bgra", 40, 30, layer)
    gc = G.to_gpu(ctx, "nv12", cw, ch, util.alloc_image("nv12", cw, ch, seed=8))
    gd = G.to_gpu(ctx, "nv12", ow, oh, util.alloc_image("nv12", ow, oh, seed=9))

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gc, kernel=K("img_clear_nv12"), blends=False)
        c = sv.runComputeKernel(c, images=[gl], target=gc, kernel=K("img_bgra_nv12"), uniforms=u, blends=True)
        c = sv.scaleLanczos(c, gd, gc)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gc, "nv12", cw, ch), canvas, "the composited canvas")
    G.assert_same(G.from_gpu(ctx, gd, "nv12", ow, oh), exp, "the resize of the canvas composited in the same pass")
