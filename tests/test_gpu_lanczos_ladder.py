"""chv_scale_lanczos_to_yuv_ladder: every rung of an encoder ladder — the renditions of one or several BGRA / RGBA
canvases of one size as NV12 or y420p pictures of up to eight sizes — in one launch per route.  Bit-exact, no tolerance, no case excluded.

The reference is the one tests/test_gpu_lanczos_to_yuv.py builds (the oracle's 4-channel Lanczos codes, then section 4.4.2 in numpy integers);
every ladder is compared with it AND with the single calls into a second set of targets.  Every target is pre-filled with seeded bytes."""
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
from test_gpu_lanczos_to_yuv import FORMATS, ORDERS, Placing, expected, target_to_gpu, to_yuv

pytestmark = pytest.mark.gpu

K = sv.defaultComputeKernelFromString
NP = {"nv12": 2, "y420p": 3}

# rungs of a 288 x 144 source: (taps, route) by launch_lanczos_to_yuv's rules
SRC = (288, 144)
RUNGS = {(288, 144): (6, "strip"), (400, 200): (6, "strip"),      # 1:1, an enlargement
         (192, 96): (10, "strip"), (191, 95): (10, "strip"),      # (odd: luma-only last column and row)
         (144, 72): (12, "strip"), (130, 64): (14, "strip"), (96, 48): (18, "strip"),
         (82, 41): (22, "strip"),                                 # a staged row of 63 vectors
         (72, 36): (24, "tile"), (101, 37): (None, "tile")}       # past the strips; unequal taps (18 / 24)
WIDE_SRC = (1100, 40)                                             # several strips with a partial last one
WIDE = [(550, 20), (733, 27), (367, 13)]                          # 12 taps, 10 taps, 18 / 20 taps (tile)
LADDERS = {
    "four_wave": (SRC, [(192, 96), (144, 72), (130, 64)]),                 # largest tap count 14: the four-wave variant
    "three_wave": (SRC, [(192, 96), (96, 48), (82, 41)]),                  # 22 taps: the three-wave variant, lean bodies beside a plain one
    "mixed": (SRC, [(144, 72), (72, 36), (101, 37), (96, 48)]),            # two launches
    "tile_only": (SRC, [(72, 36)]),
    "one_rung": (SRC, [(192, 96)]),
    "eight": (SRC, [(288, 144), (400, 200), (192, 96), (191, 95), (192, 96), (82, 41), (72, 36), (101, 37)]),      # a size twice, the 1:1 rung
    "wide": (WIDE_SRC, WIDE),
}
MIXED = LADDERS["mixed"]


def counter():
    return cv.get_counter("lanczos_ladder_launches")


def references(fmt, order, csc, src_size, sizes, n):
    """(source planes, exp[r][i]) from the shared, cached reference: sources 900 .. 900 + n - 1 of that size"""
    iw, ih = src_size
    srcs, exps = [None] * n, [[None] * n for _ in sizes]
    for r, (w, h) in enumerate(sizes):
        for i in range(n):
            srcs[i], exps[r][i] = expected(fmt, order, "random", iw, ih, w, h, 900 + i, csc)
    return srcs, exps


def fresh_targets(ctx, fmt, sizes, n, seed, place=None):
    """rungs[r][i], each pre-filled with seeded bytes"""
    put = place or (lambda f, w, h, planes: target_to_gpu(ctx, f, w, h, planes))
    return [[put(fmt, w, h, util.alloc_image(fmt, w, h, seed=seed + 16 * r + i)) for i in range(n)] for r, (w, h) in enumerate(sizes)]


def check_rungs(ctx, fmt, sizes, rungs, exps, what, singles=None, read=None):
    read = read or (lambda sample, f, w, h: G.from_gpu(ctx, sample, f, w, h))
    for r, (w, h) in enumerate(sizes):
        for i, gd in enumerate(rungs[r]):
            got = read(gd, fmt, w, h)
            G.assert_same(got, exps[r][i], f"{what}: rung {r} ({w}x{h}) of source {i} against the reference")
            if singles:
                G.assert_same(got, read(singles[r][i], fmt, w, h), f"{what}: rung {r} ({w}x{h}) of source {i} against the single call")


def run_ladder(ctx, fmt, order, csc, src_size, sizes, n, what):
    iw, ih = src_size
    srcs, exps = references(fmt, order, csc, src_size, sizes, n)
    gs = [G.to_gpu(ctx, order, iw, ih, [s]) for s in srcs]
    rungs, singles = fresh_targets(ctx, fmt, sizes, n, 3), fresh_targets(ctx, fmt, sizes, n, 1003)
    sv.usingContext(ctx, lambda c: sv.scaleLanczosToYuvLadder(c, rungs, gs if n > 1 else gs[0], colorspace=csc))
    for r in range(len(sizes)):
        for i in range(n):
            sv.usingContext(ctx, lambda c: sv.scaleLanczosToYuv(c, singles[r][i], gs[i], colorspace=csc))
    check_rungs(ctx, fmt, sizes, rungs, exps, what, singles)


def test_the_oracle_refuses_no_rung():
    """(CPU work, shared with every test below through the cache) every rung of the table has a reference"""
    for src_size, sizes in ((SRC, list(RUNGS)), (WIDE_SRC, WIDE)):
        for w, h in sizes:
            d4 = np.zeros((h, w, 4), dtype=np.uint8)
            assert O.lanczos_bgra(d4, util.alloc_image("bgra", *src_size, seed=1)[0], threads=4) == 0, (src_size, w, h)


# ---- 1. the ladders ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("k,name", list(enumerate(LADDERS)))
def test_ladder_equals_the_single_calls_and_the_reference(ctx, k, name, fmt, order, n):
    src_size, sizes = LADDERS[name]
    csc = (k + FORMATS.index(fmt) + 2 * ORDERS.index(order) + n) % 4
    run_ladder(ctx, fmt, order, csc, src_size, sizes, n, f"{name} ladder, {order} -> {fmt}, colourspace {csc}, {n} source(s)")


def test_every_rung_of_the_table_is_in_a_ladder():
    assert {s for src, sizes in LADDERS.values() if src == SRC for s in sizes} == set(RUNGS)


# ---- 2. launches -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,launches", [("four_wave", 1), ("three_wave", 1), ("tile_only", 1), ("mixed", 2), ("eight", 2)])
def test_launch_counter(ctx, name, launches):
    """the strip rungs leave in one launch, the tile rungs in one more: never more than two, whatever the rungs"""
    src_size, sizes = LADDERS[name]
    assert src_size == SRC and launches == len({RUNGS[s][1] for s in sizes})
    srcs, exps = references("nv12", "bgra", 0, src_size, sizes, 3)
    gs = [G.to_gpu(ctx, "bgra", *src_size, [s]) for s in srcs]
    rungs = fresh_targets(ctx, "nv12", sizes, 3, 5)
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosToYuvLadder(c, rungs, gs, colorspace=0))
    assert counter() - before == launches
    check_rungs(ctx, "nv12", sizes, rungs, exps, f"{name} ladder under the counter")


def header_chunk(n_rungs, planes):
    """CHV_LADDER_CHUNK of include/chipvideo.h, from the header's own numbers"""
    text = (Path(__file__).resolve().parents[1] / "include" / "chipvideo.h").read_text()
    slot = int(re.search(r"#define CHV_LADDER_SLOT_BYTES (\d+)", text).group(1))
    plane = int(re.search(r"#define CHV_LADDER_PLANE_BYTES (\d+)", text).group(1))
    assert "#define CHV_LADDER_CHUNK(n_rungs, planes) (CHV_LADDER_SLOT_BYTES / (((n_rungs) * (planes) + 1) * CHV_LADDER_PLANE_BYTES))" in text
    return slot // ((n_rungs * planes + 1) * plane)


@pytest.mark.parametrize("fmt", FORMATS)
def test_chunk_boundary(ctx, fmt):
    """one chunk plus one picture, a strip rung and a tile rung: two chunks of two launches, all rungs of a picture in one chunk"""
    src_size, sizes = (40, 24), [(20, 12), (10, 6)]
    n = header_chunk(len(sizes), NP[fmt]) + 1
    assert n > 2
    srcs, exps = references(fmt, "bgra", 0, src_size, sizes, n)
    gs = [G.to_gpu(ctx, "bgra", *src_size, [s]) for s in srcs]
    rungs, singles = fresh_targets(ctx, fmt, sizes, n, 7), fresh_targets(ctx, fmt, sizes, n, 2007)
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosToYuvLadder(c, rungs, gs, colorspace=0))
    assert counter() - before == 4
    for r in range(len(sizes)):
        sv.usingContext(ctx, lambda c: sv.LanczosToYuvBatch(list(zip(singles[r], gs)), colorspace=0).run(c))
    check_rungs(ctx, fmt, sizes, rungs, exps, f"{n} pictures into {fmt}", singles)


def test_the_ladder_object_replays(ctx):
    src_size, sizes = MIXED
    srcs, exps = references("y420p", "rgba", 3, src_size, sizes, 2)
    gs = [G.to_gpu(ctx, "rgba", *src_size, [s]) for s in srcs]
    rungs = fresh_targets(ctx, "y420p", sizes, 2, 9)
    ladder = sv.LanczosToYuvLadder(rungs, gs, colorspace=3)
    before = counter()
    sv.usingContext(ctx, lambda c: ladder.run(c))
    check_rungs(ctx, "y420p", sizes, rungs, exps, "first run")
    sv.usingContext(ctx, lambda c: ladder.run(c))
    assert counter() - before == 4
    check_rungs(ctx, "y420p", sizes, rungs, exps, "second run")


def test_null_opts_mean_bt601_limited(ctx):
    src_size, sizes = LADDERS["one_rung"]
    srcs, exps = references("nv12", "bgra", 0, src_size, sizes, 1)
    gs = G.to_gpu(ctx, "bgra", *src_size, [srcs[0]])
    rungs = fresh_targets(ctx, "nv12", sizes, 1, 11)
    d, s = sv._image_desc(rungs[0][0]), sv._image_desc(gs)
    cv.check(cv.load().chv_scale_lanczos_to_yuv_ladder(ctx.handle, C.byref(d), 1, C.byref(s), 1, None))
    check_rungs(ctx, "nv12", sizes, rungs, exps, "opts == NULL")


# ---- 3. foreign layouts ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def placing(ctx):
    p = Placing(ctx)
    yield p
    p.rec.sweep(ctx)            # every allocation downloaded completely: payload of the targets changed, nothing else, no byte of a source


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("src_layout,dst_layout", [(l, l) for l in L.LAYOUTS] + [("guarded", "skewed"), ("skewed", "guarded"), ("view", "tight"),
                                                   ("guarded", "at1p3"), ("guarded", "at4p4"), ("tight", "at2p6")])
def test_foreign_layouts(ctx, placing, fmt, src_layout, dst_layout):
    """the kernels index planes by rung and picture: every allocation is read back whole, so a wrong index shows as a changed guard byte, a
    changed source or an unchanged target"""
    src_size, sizes = MIXED
    srcs, exps = references(fmt, "bgra", 0, src_size, sizes, 2)
    gs = [placing.place("bgra", *src_size, [s], src_layout) for s in srcs]
    rungs = fresh_targets(ctx, fmt, sizes, 2, 13, place=lambda f, w, h, planes: placing.place(f, w, h, planes, dst_layout))
    sv.usingContext(ctx, lambda c: sv.scaleLanczosToYuvLadder(c, rungs, gs))
    check_rungs(ctx, fmt, sizes, rungs, exps, f"mixed ladder, sources on {src_layout}, targets on {dst_layout}", read=placing.from_gpu)


# ---- 4. inside a pass --------------------------------------------------------------------------------------------------------------------
def test_ladder_inside_a_pass_sees_the_held_composite(ctx):
    cw, ch, sizes = 128, 72, [(96, 54), (64, 36), (32, 18)]       # (the last one: 24 taps, the tile route)
    layer = util.alloc_image("nv12", 40, 30, seed=7)
    u = util.make_uniforms((cw, ch), rect=(10, 6, 60, 40), border=(2, 2, 2, 2), fill=(0.2, 0.6, 0.3, 0.7), opacity=0.8, in_size=(40, 30))
    canvas = util.alloc_image("bgra", cw, ch, seed=8)
    assert O.run_kernel("img_clear_bgra", canvas) == 0
    assert O.run_kernel("img_nv12_bgra", canvas, layer, u) == 0
    exps = []
    for w, h in sizes:
        d4 = np.zeros((h, w, 4), dtype=np.uint8)
        assert O.lanczos_bgra(d4, np.ascontiguousarray(canvas[0]), threads=4) == 0
        exps.append([to_yuv("nv12", "bgra", d4, 1)])
    gl = G.to_gpu(ctx, "nv12", 40, 30, layer)
    gc = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=8))
    rungs = fresh_targets(ctx, "nv12", sizes, 1, 15)

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gc, kernel=K("img_clear_bgra"), blends=False)
        c = sv.runComputeKernel(c, images=[gl], target=gc, kernel=K("img_nv12_bgra"), uniforms=u, blends=True)
        c = sv.scaleLanczosToYuvLadder(c, rungs, gc, colorspace=1)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gc, "bgra", cw, ch), canvas, "the composited canvas")
    check_rungs(ctx, "nv12", sizes, rungs, exps, "the ladder of the canvas composited in the same pass")


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------------
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
            G.assert_same(G.from_gpu(self.ctx, g, fmt, w, h), planes, f"{what}: a refused ladder wrote to a {w}x{h} {fmt} picture")


def status(ctx, rung_descs, src_descs, n_rungs=None, n=None):
    """the status of the C call for rungs given as lists of descriptors (rung_descs[r][i]); `n_rungs` / `n` override the counts"""
    flat = [d for rung in rung_descs for d in rung]
    d = (cv.Image * max(1, len(flat)))(*flat)
    s = (cv.Image * max(1, len(src_descs)))(*src_descs)
    opts = cv.KernelOpts(colorspace=0)
    rc = cv.load().chv_scale_lanczos_to_yuv_ladder(ctx.handle, d, len(rung_descs) if n_rungs is None else n_rungs, s, len(src_descs) if n is None else n, C.byref(opts))
    if rc == 0:
        return "success"
    with pytest.raises(sv.ComputeError) as e:
        cv.check(rc)
    return e.value.case


def test_errors_leave_every_rung_unchanged(ctx):
    pic, desc = Pictures(ctx), sv._image_desc
    src = [pic("bgra", 64, 36), pic("bgra", 64, 36)]
    nv = [[pic("nv12", 32, 18), pic("nv12", 32, 18)], [pic("nv12", 16, 10), pic("nv12", 16, 10)]]
    yp = [pic("y420p", 16, 10), pic("y420p", 16, 10)]
    D = lambda rows: [[desc(g) for g in row] for row in rows]      # noqa: E731
    S = lambda row: [desc(g) for g in row]                         # noqa: E731
    nine = [[pic("nv12", 8 + 2 * r, 6)] for r in range(9)]
    assert status(ctx, D(nine), S(src[:1])) == "invalidValue"                                   # n_rungs = 9
    assert status(ctx, D(nv), S(src), n_rungs=-1) == "invalidValue"
    assert status(ctx, D(nv), S(src), n=-1) == "invalidValue"
    lib, opts = cv.load(), cv.KernelOpts(colorspace=0)
    with pytest.raises(sv.ComputeError) as e:                                                   # a NULL list with non-zero counts
        cv.check(lib.chv_scale_lanczos_to_yuv_ladder(ctx.handle, None, 1, C.byref(desc(src[0])), 1, C.byref(opts)))
    assert e.value.case == "invalidValue"
    with pytest.raises(sv.ComputeError) as e:
        cv.check(lib.chv_scale_lanczos_to_yuv_ladder(ctx.handle, C.byref(desc(nv[0][0])), 1, None, 1, C.byref(opts)))
    assert e.value.case == "invalidValue"
    assert status(ctx, D([nv[0], yp]), S(src)) == "invalidValue"                                # mixed target formats
    assert status(ctx, D([yp, nv[0]]), S(src)) == "invalidValue"
    rgba = desc(src[1])
    rgba.format = cv.FMT_RGBA
    assert desc(src[0]).format == cv.FMT_BGRA
    assert status(ctx, D(nv), [desc(src[0]), rgba]) == "invalidValue"                           # mixed source formats
    assert status(ctx, D([nv[0], [nv[1][0], nv[0][1]]]), S(src)) == "invalidValue"              # two sizes inside a rung
    assert status(ctx, D(nv), S([src[0], pic("bgra", 80, 36)])) == "invalidValue"               # two source sizes
    bad = D(nv)
    bad[1][1].planes[1].width = 7                                                               # a bad chroma plane in the last rung
    assert status(ctx, bad, S(src)) == "badTarget"
    far = D(nv)
    far[1][1].planes[1].height = 1 << 20                                                        # ... one whose extent leaves its buffer
    assert status(ctx, far, S(src)) == "badTarget"
    assert status(ctx, D(nv), S([src[0], pic("nv12", 64, 36)])) == "invalidValue"               # an NV12 source among BGRA ones: the list's mistake
    assert status(ctx, D([nv[0][:1], nv[1][:1]]), S([pic("nv12", 64, 36)])) == "badInputData"   # an NV12 source
    big = pic("bgra", 96, 96)                                                                   # the LAST rung is 24:1: the 160 KB rule
    first, tiny = pic("nv12", 48, 48), pic("nv12", 4, 4)
    assert status(ctx, D([[first], [tiny]]), S([big])) == "invalidValue"
    pic.unchanged("errors")
    # (the lists the refusals were made from are good ladders: every refusal above is the one it names)
    assert status(ctx, D(nv), S(src)) == "success"
    assert status(ctx, D([[first]]), S([big])) == "success"


def test_empty_ladders_are_noops(ctx):
    pic, desc = Pictures(ctx), sv._image_desc
    src, dst = pic("bgra", 64, 36), pic("nv12", 32, 18)
    before = counter()
    assert status(ctx, [[desc(dst)]], [desc(src)], n_rungs=0) == "success"
    assert status(ctx, [[desc(dst)]], [desc(src)], n=0) == "success"
    lib = cv.load()
    cv.check(lib.chv_scale_lanczos_to_yuv_ladder(ctx.handle, None, 0, None, 0, None))
    cv.check(lib.chv_scale_lanczos_to_yuv_ladder(ctx.handle, None, 0, None, 3, None))
    cv.check(lib.chv_scale_lanczos_to_yuv_ladder(ctx.handle, None, 3, None, 0, None))
    assert sv.scaleLanczosToYuvLadder(ctx, [], []) is ctx
    assert counter() == before
    pic.unchanged("an empty ladder")
