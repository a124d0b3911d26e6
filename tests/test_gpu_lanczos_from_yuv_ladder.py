"""chv_scale_lanczos_from_yuv_ladder: every BGRA / RGBA rendition of every NV12 or y420p picture of a list in one
launch per route.  Bit-exact, no tolerance, no case excluded.

The expectation is tests/test_gpu_lanczos_from_yuv.py's: the oracle's 4-channel Lanczos gives the codes of the three logical planes at a
rung's size, section 4.2 in numpy the pixels.  Every target is compared with that expectation AND with the bytes of the single call; every
target is pre-filled with seeded bytes and whole planes are compared."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import gpuutil as G
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv
from test_gpu_lanczos_from_yuv import Pictures, _case_of, case, codes, expected, packed, pixels, source_to_gpu
from test_gpu_lanczos_yuv import Placing

pytestmark = pytest.mark.gpu

K = sv.defaultComputeKernelFromString
SOURCES = ["nv12", "y420p"]
TARGETS = ["bgra", "rgba"]
# one source size, four rungs: 10 / 6 taps (the short strip body), 22 / 12 (the strip route's edge), 24 (the tile route), an enlargement
SRC, RUNGS = (288, 144), [(192, 96), (82, 41), (72, 36), (400, 200)]


def counter():
    return cv.get_counter("lanczos_from_yuv_ladder_launches")


def singles():
    return cv.get_counter("lanczos_from_yuv_launches")


@functools.lru_cache(maxsize=None)
def ladder_case(iw, ih, rungs, n):
    """n sources of one size that differ (batch_case's: picture i is the seeded case with i added to every byte) as (Y, Cb, Cr), and the
    codes of every picture at every rung's size: computed once, shared and left unchanged by every test that names the ladder"""
    (y, cb, cr), _ = case(iw, ih, rungs[0][0], rungs[0][1], "random")
    srcs = [(y + np.uint8(i % 256), cb + np.uint8(3 * i % 256), cr + np.uint8(5 * i % 256)) for i in range(n)]
    cod = [[codes(*s, ow, oh) for (ow, oh) in rungs] for s in srcs]
    for s in srcs:
        for a in s:
            a.setflags(write=False)
    return srcs, cod


def run_ladder(ctx, sfmt, dfmt, iw, ih, rungs, n, csc, launches, what, compare_single=True):
    """the ladder of `rungs` over n pictures against the reference and against the single calls; returns the downloaded targets [r][i]"""
    rungs = tuple(rungs)
    srcs, cod = ladder_case(iw, ih, rungs, n)
    gs = [source_to_gpu(ctx, sfmt, iw, ih, packed(sfmt, *s)) for s in srcs]
    gl, g1 = ([[G.to_gpu(ctx, dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=seed + 16 * r + i)) for i in range(n)]
               for r, (ow, oh) in enumerate(rungs)] for seed in (500, 900))
    before, single_before = counter(), singles()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuvLadder(c, gl, gs, colorspace=csc))
    assert counter() - before == launches, f"{what}: {counter() - before} launches, not {launches}"
    assert singles() == single_before, "the ladder does not touch the single entry's counter"
    got = [[G.from_gpu(ctx, gl[r][i], dfmt, ow, oh) for i in range(n)] for r, (ow, oh) in enumerate(rungs)]
    for r, (ow, oh) in enumerate(rungs):
        for i in range(n):
            G.assert_same(got[r][i], pixels(dfmt, csc, *cod[i][r]), f"{what}: rung {r} ({ow}x{oh}), picture {i}, against the reference")
            if compare_single:
                sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuv(c, g1[r][i], gs[i], colorspace=csc))
                G.assert_same(got[r][i], G.from_gpu(ctx, g1[r][i], dfmt, ow, oh), f"{what}: rung {r} ({ow}x{oh}), picture {i}, against the single call")
    assert counter() - before == launches
    return got


# ---- 1. all routes in one ladder ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dfmt", TARGETS)
@pytest.mark.parametrize("sfmt", SOURCES)
def test_all_routes_in_one_ladder(ctx, sfmt, dfmt):
    """three strip rungs (one of them at the strip route's edge: <22, .>) in one launch, the tile rung in one more"""
    csc = (SOURCES.index(sfmt) + 2 * TARGETS.index(dfmt) + 1) % 4
    run_ladder(ctx, sfmt, dfmt, *SRC, RUNGS, 3, csc, 2, f"{sfmt} -> {dfmt}, all routes")


# ---- 2. <12, .> alone, 3. the tile route alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfmt,dfmt", [("nv12", "rgba"), ("y420p", "bgra")])
def test_short_strip_rungs_alone(ctx, sfmt, dfmt):
    run_ladder(ctx, sfmt, dfmt, *SRC, [(192, 96), (400, 200), (288, 144)], 2, 0, 1, f"{sfmt} -> {dfmt}, <12> alone")


@pytest.mark.parametrize("sfmt,dfmt", [("nv12", "bgra"), ("y420p", "rgba")])
def test_tile_rungs_alone(ctx, sfmt, dfmt):
    run_ladder(ctx, sfmt, dfmt, *SRC, [(72, 36), (36, 18)], 2, 3, 1, f"{sfmt} -> {dfmt}, tile route alone")


# ---- 4. eight rungs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfmt,dfmt", [("nv12", "bgra"), ("y420p", "rgba")])
def test_eight_rungs(ctx, sfmt, dfmt):
    """two rungs of one size hold identical bytes; one rung has the source's size"""
    iw, ih = 96, 54
    rungs = [(64, 36), (96, 54), (48, 27), (64, 36), (130, 70), (33, 19), (20, 12), (12, 6)]
    got = run_ladder(ctx, sfmt, dfmt, iw, ih, rungs, 2, 1, 2, f"{sfmt} -> {dfmt}, eight rungs")
    for i in range(2):
        G.assert_same(got[0][i], got[3][i], f"rungs 0 and 3 have one size, picture {i}")


# ---- 5. edges of the decode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfmt,dfmt", [("nv12", "bgra"), ("y420p", "rgba")])
def test_several_strips_and_row_chunks(ctx, sfmt, dfmt):
    """several strips with a partial last one, several row chunks, an odd last row"""
    run_ladder(ctx, sfmt, dfmt, 1000, 202, [(500, 101), (333, 67), (1100, 222)], 1, 2, 1, f"{sfmt} -> {dfmt}, 1000x202")


@pytest.mark.parametrize("sfmt", SOURCES)
def test_smallest_sources(ctx, sfmt):
    run_ladder(ctx, sfmt, "bgra", 2, 2, [(7, 5), (1, 1)], 2, 0, 1, f"{sfmt}, 2x2")
    run_ladder(ctx, sfmt, "rgba", 1, 1, [(5, 3)], 1, 3, 1, f"{sfmt}, 1x1")          # (source_to_gpu describes the 1 x 1 chroma planes by hand)


# ---- 6. one real size, once ---------------------------------------------------------------------------------------------------------------
def test_one_real_size(ctx):
    """1920x1080 NV12 -> BGRA at four sizes; the last rung (36 taps) takes the tile route"""
    run_ladder(ctx, "nv12", "bgra", 1920, 1080, [(1280, 720), (854, 480), (640, 360), (320, 180)], 1, 1, 2, "1080p")


# ---- 7. chunks ------------------------------------------------------------------------------------------------------------------------------
def chunk_macro(n_rungs, src_planes, slot=5984, plane=24):
    return slot // ((n_rungs + src_planes) * plane)


def test_the_macro_is_the_headers():
    header = (Path(__file__).resolve().parents[1] / "include" / "chipvideo.h").read_text()
    assert re.search(r"#define CHV_FROM_YUV_LADDER_CHUNK\(n_rungs, src_planes\) \\\n\s*\(CHV_LADDER_SLOT_BYTES / \(\(\(n_rungs\) \+ \(src_planes\)\) \* CHV_LADDER_PLANE_BYTES\)\)",
                     header)
    assert "#define CHV_LADDER_SLOT_BYTES 5984" in header and "#define CHV_LADDER_PLANE_BYTES 24" in header
    assert (chunk_macro(1, 2), chunk_macro(1, 3)) == (83, 62), "one rung: the batch's counts"
    assert (chunk_macro(8, 2), chunk_macro(8, 3)) == (24, 22)


@pytest.mark.parametrize("sfmt,n", [("nv12", 25), ("y420p", 23)])
def test_one_picture_more_than_a_chunk(ctx, sfmt, n):
    """8 rungs that all take the strip route: CHV_FROM_YUV_LADDER_CHUNK(8, planes) + 1 pictures leave in exactly two launches"""
    assert n == chunk_macro(8, 2 if sfmt == "nv12" else 3) + 1
    rungs = [(8, 8), (12, 12), (16, 16), (20, 20), (24, 12), (10, 6), (32, 32), (9, 9)]
    run_ladder(ctx, sfmt, "bgra", 16, 16, rungs, n, 2, 2, f"{n} {sfmt} pictures", compare_single=False)


# ---- 8. no-ops ------------------------------------------------------------------------------------------------------------------------------
def test_empty_ladders_are_noops(ctx):
    pic = Pictures(ctx)
    s, d = sv._image_desc(pic("nv12", 16, 16)), sv._image_desc(pic("bgra", 8, 8))
    before = counter()
    lib = cv.load()
    cv.check(lib.chv_scale_lanczos_from_yuv_ladder(ctx.handle, None, 0, None, 0, None))
    cv.check(lib.chv_scale_lanczos_from_yuv_ladder(ctx.handle, C.byref(d), 0, C.byref(s), 1, None))
    cv.check(lib.chv_scale_lanczos_from_yuv_ladder(ctx.handle, C.byref(d), 1, C.byref(s), 0, None))
    cv.check(lib.chv_scale_lanczos_from_yuv_ladder(ctx.handle, None, 3, None, 0, None))
    assert sv.scaleLanczosFromYuvLadder(ctx, [], []) is ctx
    assert sv.scaleLanczosFromYuvLadder(ctx, [[], []], []) is ctx
    assert counter() == before
    pic.unchanged("no-ops")


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------------
def ladder(ctx, rungs, ss, csc=None):
    """rungs: [[desc per source] per rung]"""
    n, flat = len(ss), [d for rung in rungs for d in rung]
    d, s = (cv.Image * max(1, len(flat)))(*flat), (cv.Image * max(1, n))(*ss)
    opts = None if csc is None else C.byref(cv.KernelOpts(colorspace=csc))
    return _case_of(cv.load().chv_scale_lanczos_from_yuv_ladder(ctx.handle, d, len(rungs), s, n, opts))


def test_errors_leave_every_target_of_every_rung_unchanged(ctx):
    """host refusals only: nothing is launched in any of them"""
    pic, desc = Pictures(ctx), sv._image_desc
    nv = [pic("nv12", 96, 96) for _ in range(2)]
    yp = [pic("y420p", 96, 96) for _ in range(2)]
    big = [pic("bgra", 64, 64) for _ in range(2)]
    small = [pic("bgra", 32, 32) for _ in range(2)]
    rg = [pic("rgba", 32, 32) for _ in range(2)]
    good = [[desc(g) for g in big], [desc(g) for g in small]]
    S = [desc(g) for g in nv]
    before, single_before = counter(), singles()
    lib = cv.load()
    # the counts and the lists
    d9 = (cv.Image * 18)(*([desc(big[0])] * 18))
    s2 = (cv.Image * 2)(*S)
    assert _case_of(lib.chv_scale_lanczos_from_yuv_ladder(ctx.handle, d9, 9, s2, 2, None)) == "invalidValue"           # CHV_LADDER_MAX_RUNGS is 8
    assert _case_of(lib.chv_scale_lanczos_from_yuv_ladder(ctx.handle, d9, -1, s2, 2, None)) == "invalidValue"
    assert _case_of(lib.chv_scale_lanczos_from_yuv_ladder(ctx.handle, d9, 2, s2, -1, None)) == "invalidValue"
    assert _case_of(lib.chv_scale_lanczos_from_yuv_ladder(ctx.handle, None, 2, s2, 2, None)) == "invalidValue"
    assert _case_of(lib.chv_scale_lanczos_from_yuv_ladder(ctx.handle, d9, 2, None, 2, None)) == "invalidValue"
    # one target format, one source format and size, one size per rung
    assert ladder(ctx, [good[0], [desc(small[0]), desc(rg[1])]], S) == "invalidValue"                  # two target orders
    assert ladder(ctx, [good[0], [desc(small[0]), desc(pic("nv12", 32, 32))]], S) == "invalidValue"    # a target of another format
    assert ladder(ctx, good, [desc(nv[0]), desc(yp[1])]) == "invalidValue"                             # two source formats
    assert ladder(ctx, good, [desc(nv[0]), desc(pic("nv12", 98, 96))]) == "invalidValue"               # two source sizes
    assert ladder(ctx, [good[0], [desc(small[0]), desc(pic("bgra", 30, 32))]], S) == "invalidValue"    # two sizes in the last rung
    # one picture: the single call's statuses
    assert ladder(ctx, [[desc(pic("nv12", 32, 32)), desc(pic("nv12", 32, 32))]], S) == "badTarget"
    far = desc(small[1])
    far.planes[0].height = 1 << 20                                              # the last target: a plane extent outside its buffer
    assert ladder(ctx, [good[0], [desc(small[0]), far]], S) == "badTarget"
    two = desc(small[1])
    two.n_planes = 2
    assert ladder(ctx, [good[0], [desc(small[0]), two]], S) == "badTarget"
    assert ladder(ctx, good, [desc(pic("bgra", 96, 96)), desc(pic("bgra", 96, 96))]) == "badInputData"
    for src in (nv, yp):
        bad = desc(src[1])                                                      # a wrong chroma plane size in the last source
        for p in range(1, bad.n_planes):
            bad.planes[p].width = bad.planes[p].width - 1
        assert ladder(ctx, good, [desc(src[0]), bad]) == "badInputData"
    skew = desc(yp[1])                                                          # a y420p picture with unequal chroma planes
    skew.planes[2].height = skew.planes[2].height - 1
    assert ladder(ctx, good, [desc(yp[0]), skew]) == "badInputData"
    comps = desc(nv[1])
    comps.planes[1].components = 1
    assert ladder(ctx, good, [desc(nv[0]), comps]) == "badInputData"
    # a refused LAST rung after valid ones: 30:1 trips the 160 KB rule on the luma plane's own sizes
    wide = [pic("nv12", 120, 96) for _ in range(2)]
    tiny = [pic("bgra", 4, 4) for _ in range(2)]
    assert ladder(ctx, [good[0], good[1], [desc(g) for g in tiny]], [desc(g) for g in wide]) == "invalidValue"
    assert ladder(ctx, [[desc(g) for g in tiny]], [desc(g) for g in wide], csc=2) == "invalidValue"
    assert counter() == before and singles() == single_before, "a refused ladder launched something"
    pic.unchanged("errors")
    # (the pictures the refusals were made from make good ladders: every refusal above is the one it names)
    assert ladder(ctx, good, S) == "success"
    assert ladder(ctx, [good[0]], [desc(g) for g in wide], csc=3) == "success"
    assert ladder(ctx, [[desc(g) for g in rg]], [desc(g) for g in yp], csc=1) == "success"
    assert counter() - before == 3


# ---- 10. foreign layouts -------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def placing(ctx):
    p = Placing(ctx)
    yield p
    p.rec.sweep(ctx)            # every allocation downloaded completely: payload of the targets changed, nothing else, no byte of a source


@pytest.mark.parametrize("sfmt,dfmt,src_layout,dst_layout", [("nv12", "bgra", "view", "at12p8"), ("y420p", "rgba", "guarded", "skewed")])
def test_foreign_layouts(ctx, placing, sfmt, dfmt, src_layout, dst_layout):
    """the ladder of (1) on views of larger parents behind guard bands; each allocation is read back whole"""
    n, csc, rungs = 2, 1, tuple(RUNGS)
    srcs, cod = ladder_case(*SRC, rungs, 3)
    gs = [placing.place(sfmt, *SRC, packed(sfmt, *srcs[i]), src_layout) for i in range(n)]
    gd = [[placing.place(dfmt, ow, oh, util.alloc_image(dfmt, ow, oh, seed=11 + 8 * r + i), dst_layout) for i in range(n)] for r, (ow, oh) in enumerate(rungs)]
    p = placing.rec.placement(gd[0][0]).planes[0]
    assert p.offset % 4 == 0 and p.offset % 16 != 0 and p.pitch % 16 != 0
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuvLadder(c, gd, gs, colorspace=csc))
    assert counter() - before == 2
    for r, (ow, oh) in enumerate(rungs):
        for i in range(n):
            G.assert_same(placing.from_gpu(gd[r][i], dfmt, ow, oh), pixels(dfmt, csc, *cod[i][r]),
                          f"{sfmt} -> {dfmt} rung {r}, picture {i}, {src_layout} -> {dst_layout}")


# ---- 11. inside a pass ---------------------------------------------------------------------------------------------------------------------
def test_ladder_inside_a_pass_sees_the_held_composite(ctx):
    cw, ch, rungs = 128, 72, [(64, 36), (96, 54), (24, 14)]
    layer = util.alloc_image("bgra", 40, 30, seed=7)
    u = util.make_uniforms((cw, ch), rect=(10, 6, 60, 40), border=(2, 2, 2, 2), fill=(0.2, 0.6, 0.3, 0.7), opacity=0.8, in_size=(40, 30))
    canvas = util.alloc_image("nv12", cw, ch, seed=8)
    assert O.run_kernel("img_clear_nv12", canvas) == 0
    assert O.run_kernel("img_bgra_nv12", canvas, layer, u) == 0
    gl = G.to_gpu(ctx, "bgra", 40, 30, layer)
    gc = G.to_gpu(ctx, "nv12", cw, ch, util.alloc_image("nv12", cw, ch, seed=8))
    gd = [G.to_gpu(ctx, "bgra", ow, oh, util.alloc_image("bgra", ow, oh, seed=9 + r)) for r, (ow, oh) in enumerate(rungs)]

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gc, kernel=K("img_clear_nv12"), blends=False)
        c = sv.runComputeKernel(c, images=[gl], target=gc, kernel=K("img_bgra_nv12"), uniforms=u, blends=True)
        c = sv.scaleLanczosFromYuvLadder(c, gd, gc)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gc, "nv12", cw, ch), canvas, "the composited canvas")
    for r, (ow, oh) in enumerate(rungs):
        G.assert_same(G.from_gpu(ctx, gd[r], "bgra", ow, oh), expected("nv12", canvas, ow, oh, "bgra", 0),
                      f"rung {r}: the BGRA rendition of the canvas composited in the same pass")
