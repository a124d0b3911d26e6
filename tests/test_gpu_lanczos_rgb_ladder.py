"""chv_scale_lanczos_rgb_ladder: every rendition of every BGRA / RGBA plane of a list in one launch per route.
Bit-exact, no tolerance, no byte excluded.

The expectation is the oracle's 4-channel Lanczos (orc_lanczos_bgra) per (rung, picture).  Every target is compared with that expectation AND
with the bytes of the single call; every target is pre-filled with seeded bytes and whole planes are compared."""
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
from test_gpu_lanczos_from_yuv import Pictures, _case_of
from test_gpu_lanczos_yuv import Placing

pytestmark = pytest.mark.gpu

K = sv.defaultComputeKernelFromString
ORDERS = ["bgra", "rgba"]
# one source size, six rungs: 10 taps (<12> class), 22 / 22 at nv = 63 (the strip route's edge), 24 (tile), an enlargement (6), and two rungs
# whose axes differ — tx 10, ty 22 and tx 22, ty 10: strip here, tile in the single call
SRC, RUNGS = (288, 144), [(192, 96), (82, 41), (72, 36), (400, 200), (192, 41), (82, 96)]


def counter():
    return cv.get_counter("lanczos_rgb_ladder_launches")


OTHERS = ["lanczos_ladder_launches", "lanczos_planar_ladder_launches", "lanczos_420_ladder_launches", "lanczos_from_yuv_launches",
          "lanczos_from_yuv_ladder_launches"]


def others():
    return [cv.get_counter(n) for n in OTHERS]


def taps(i, o):
    return 2 * int(np.ceil(3 * max(i / o, 1.0)))


def row_vectors(sw, dw, t):
    return (int(63 * (sw / dw)) + 1 + 3 + t + 3) // 4 + 1


def strip_route(sw, sh, dw, dh):
    """the routing rule, restated from its three conditions"""
    tx, ty = taps(sw, dw), taps(sh, dh)
    return max(tx, ty) <= 22 and sw >= 4 and row_vectors(sw, dw, tx) <= 64


def test_the_named_rungs_take_the_routes_they_are_named_for():
    assert [(taps(288, w), taps(144, h)) for w, h in RUNGS] == [(10, 10), (22, 22), (24, 24), (6, 6), (10, 22), (22, 10)]
    assert row_vectors(288, 82, 22) == 63
    assert [strip_route(*SRC, w, h) for w, h in RUNGS] == [True, True, False, True, True, True]
    assert taps(288, 79) == 22 and row_vectors(288, 79, 22) == 65 and not strip_route(*SRC, 79, 40)
    assert taps(1080, 180) == 36


def oracle_resize(src, ow, oh):
    exp = np.zeros((oh, ow, 4), dtype=np.uint8)
    assert O.lanczos_bgra(exp, np.ascontiguousarray(src), threads=4) == 0, f"oracle refused {src.shape[1]}x{src.shape[0]} -> {ow}x{oh}"
    return exp


@functools.lru_cache(maxsize=None)
def ladder_case(iw, ih, rungs, n):
    """n sources of one size that differ (picture i is the seeded case with i added to every byte) and the expectation of every picture at
    every rung's size: computed once, shared and left unchanged by every test that names the ladder"""
    base = util.alloc_image("bgra", iw, ih, seed=0x5EED + iw * 7 + ih)[0]
    srcs = [base + np.uint8((37 * i) % 256) for i in range(n)]
    exp = [[oracle_resize(s, ow, oh) for (ow, oh) in rungs] for s in srcs]
    for s in srcs:
        s.setflags(write=False)
    for e in exp:
        for a in e:
            a.setflags(write=False)
    return srcs, exp


def run_ladder(ctx, fmt, iw, ih, rungs, n, launches, what, compare_single=True):
    """the ladder of `rungs` over n pictures against the reference and against the single calls; returns the downloaded targets [r][i]"""
    rungs = tuple(rungs)
    srcs, exp = ladder_case(iw, ih, rungs, n)
    gs = [G.to_gpu(ctx, fmt, iw, ih, [s]) for s in srcs]
    gl, g1 = ([[G.to_gpu(ctx, fmt, ow, oh, util.alloc_image(fmt, ow, oh, seed=seed + 16 * r + i)) for i in range(n)]
               for r, (ow, oh) in enumerate(rungs)] for seed in (500, 900))
    before, others_before = counter(), others()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosRgbLadder(c, gl, gs))
    print(f"{what}: {counter() - before} launches")
    assert counter() - before == launches, f"{what}: {counter() - before} launches, not {launches}"
    assert others() == others_before, "the ladder touches no counter of another entry"
    got = [[G.from_gpu(ctx, gl[r][i], fmt, ow, oh) for i in range(n)] for r, (ow, oh) in enumerate(rungs)]
    for r, (ow, oh) in enumerate(rungs):
        for i in range(n):
            G.assert_same(got[r][i], [exp[i][r]], f"{what}: rung {r} ({ow}x{oh}), picture {i}, against the reference")
            if compare_single:
                sv.usingContext(ctx, lambda c: sv.scaleLanczos(c, g1[r][i], gs[i]))
                G.assert_same(got[r][i], G.from_gpu(ctx, g1[r][i], fmt, ow, oh), f"{what}: rung {r} ({ow}x{oh}), picture {i}, against the single call")
    assert counter() - before == launches
    return got


# ---- 1. all routes in one ladder ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ORDERS)
def test_all_routes_in_one_ladder(ctx, fmt):
    """five strip rungs (one at the strip route's edge, two with unequal tap counts: <22>) in one launch, the tile rung in one more"""
    run_ladder(ctx, fmt, *SRC, RUNGS, 3, 2, f"{fmt}, all routes")


# ---- 2. <12> alone, 3. the tile route alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ORDERS)
def test_short_strip_rungs_alone(ctx, fmt):
    run_ladder(ctx, fmt, *SRC, [(192, 96), (400, 200), (288, 144)], 2, 1, f"{fmt}, <12> alone")


@pytest.mark.parametrize("fmt", ORDERS)
def test_tile_rungs_alone(ctx, fmt):
    """79x40 has 22 taps but a staged row of 65 vectors: the tile route by the row rule"""
    run_ladder(ctx, fmt, *SRC, [(72, 36), (36, 18), (79, 40)], 2, 1, f"{fmt}, tile route alone")


# ---- 4. eight rungs ------------------------------------------------------------------------------------------------------------------------
def test_eight_rungs(ctx):
    """two rungs of one size hold identical bytes; one rung has the source's size"""
    iw, ih = 96, 54
    rungs = [(64, 36), (96, 54), (48, 27), (64, 36), (130, 70), (33, 19), (20, 12), (12, 6)]
    routes = {strip_route(iw, ih, w, h) for w, h in rungs}
    got = run_ladder(ctx, "bgra", iw, ih, rungs, 2, len(routes), "eight rungs")
    for i in range(2):
        G.assert_same(got[0][i], got[3][i], f"rungs 0 and 3 have one size, picture {i}")


# ---- 5. edges of the decode ---------------------------------------------------------------------------------------------------------------
def test_several_strips_and_row_chunks(ctx):
    """several strips with a partial last one, several row chunks, an odd last row"""
    run_ladder(ctx, "rgba", 1000, 202, [(500, 101), (333, 67), (1100, 222)], 1, 1, "1000x202")


# ---- 6. smallest sources ------------------------------------------------------------------------------------------------------------------
def test_smallest_sources(ctx):
    """src.w < 4: the tile route"""
    run_ladder(ctx, "bgra", 2, 2, [(7, 5), (1, 1)], 2, 1, "2x2")
    run_ladder(ctx, "rgba", 1, 1, [(5, 3)], 1, 1, "1x1")


# ---- 7. one real size, once ---------------------------------------------------------------------------------------------------------------
def test_one_real_size(ctx):
    """1920x1080 at four sizes; the last rung (36 taps) takes the tile route"""
    run_ladder(ctx, "bgra", 1920, 1080, [(1280, 720), (854, 480), (640, 360), (320, 180)], 1, 2, "1080p")


# ---- 8. chunks ------------------------------------------------------------------------------------------------------------------------------
def chunk_macro(n_rungs, slot=5984, plane=24):
    return slot // ((n_rungs + 1) * plane)


def test_the_macro_is_the_headers():
    header = (Path(__file__).resolve().parents[1] / "include" / "chipvideo.h").read_text()
    assert re.search(r"#define CHV_RGB_LADDER_CHUNK\(n_rungs\) \(CHV_LADDER_SLOT_BYTES / \(\(\(n_rungs\) \+ 1\) \* CHV_LADDER_PLANE_BYTES\)\)", header)
    assert "#define CHV_LADDER_SLOT_BYTES 5984" in header and "#define CHV_LADDER_PLANE_BYTES 24" in header
    assert (chunk_macro(1), chunk_macro(8)) == (124, 27)


def test_one_picture_more_than_a_chunk(ctx):
    """8 rungs that all take the strip route: CHV_RGB_LADDER_CHUNK(8) + 1 pictures leave in exactly two launches"""
    n = chunk_macro(8) + 1
    assert n == 28
    rungs = [(8, 8), (12, 12), (16, 16), (20, 20), (24, 12), (10, 6), (32, 32), (9, 9)]
    assert all(strip_route(16, 16, w, h) for w, h in rungs)
    run_ladder(ctx, "bgra", 16, 16, rungs, n, 2, f"{n} pictures", compare_single=False)


# ---- 9. no-ops and errors -------------------------------------------------------------------------------------------------------------------
def test_empty_ladders_are_noops(ctx):
    pic = Pictures(ctx)
    s, d = sv._image_desc(pic("bgra", 16, 16)), sv._image_desc(pic("bgra", 8, 8))
    before = counter()
    lib = cv.load()
    cv.check(lib.chv_scale_lanczos_rgb_ladder(ctx.handle, None, 0, None, 0))
    cv.check(lib.chv_scale_lanczos_rgb_ladder(ctx.handle, C.byref(d), 0, C.byref(s), 1))
    cv.check(lib.chv_scale_lanczos_rgb_ladder(ctx.handle, C.byref(d), 1, C.byref(s), 0))
    cv.check(lib.chv_scale_lanczos_rgb_ladder(ctx.handle, None, 3, None, 0))
    assert sv.scaleLanczosRgbLadder(ctx, [], []) is ctx
    assert sv.scaleLanczosRgbLadder(ctx, [[], []], []) is ctx
    assert counter() == before
    pic.unchanged("no-ops")


def ladder(ctx, rungs, ss):
    """rungs: [[desc per source] per rung]"""
    n, flat = len(ss), [d for rung in rungs for d in rung]
    d, s = (cv.Image * max(1, len(flat)))(*flat), (cv.Image * max(1, n))(*ss)
    return _case_of(cv.load().chv_scale_lanczos_rgb_ladder(ctx.handle, d, len(rungs), s, n))


def launch_lanczos_refuses(sw, sh, dw, dh):
    """launch_lanczos's formula: the 8 x 4 tile's staged source beyond 160 KB"""
    tx, ty = taps(sw, dw), taps(sh, dh)
    max_rows = int(3 * (sh / dh) + 2) + ty
    max_cols = (int(7 * (sw / dw) + 2) + tx + 3) & ~3
    return max_rows * 8 * 16 + max_rows * max_cols * 4 > 160 * 1024


def test_errors_leave_every_target_of_every_rung_unchanged(ctx):
    """host refusals only: nothing is launched in any of them"""
    pic, desc = Pictures(ctx), sv._image_desc
    src = [pic("bgra", 96, 96) for _ in range(2)]
    big = [pic("bgra", 64, 64) for _ in range(2)]
    small = [pic("rgba", 32, 32) for _ in range(2)]
    good = [[desc(g) for g in big], [desc(g) for g in small]]
    S = [desc(g) for g in src]
    before, others_before = counter(), others()
    lib = cv.load()
    # the counts and the lists
    d9 = (cv.Image * 18)(*([desc(big[0])] * 18))
    s2 = (cv.Image * 2)(*S)
    assert _case_of(lib.chv_scale_lanczos_rgb_ladder(ctx.handle, d9, 9, s2, 2)) == "invalidValue"           # CHV_LADDER_MAX_RUNGS is 8
    assert _case_of(lib.chv_scale_lanczos_rgb_ladder(ctx.handle, d9, -1, s2, 2)) == "invalidValue"
    assert _case_of(lib.chv_scale_lanczos_rgb_ladder(ctx.handle, d9, 2, s2, -1)) == "invalidValue"
    assert _case_of(lib.chv_scale_lanczos_rgb_ladder(ctx.handle, None, 2, s2, 2)) == "invalidValue"
    assert _case_of(lib.chv_scale_lanczos_rgb_ladder(ctx.handle, d9, 2, None, 2)) == "invalidValue"
    # a target that is not exactly one plane of 4 components; a plane that fails a plane_to_device check — in the LAST rung, after valid ones
    for fmt in ("nv12", "y420p"):
        assert ladder(ctx, [good[0], [desc(small[0]), desc(pic(fmt, 32, 32))]], S) == "badTarget"
    two = desc(small[1])
    two.n_planes = 2
    assert ladder(ctx, [good[0], [desc(small[0]), two]], S) == "badTarget"
    comps = desc(small[1])
    comps.planes[0].components = 1
    assert ladder(ctx, [good[0], [desc(small[0]), comps]], S) == "badTarget"
    far = desc(small[1])
    far.planes[0].height = 1 << 20                                              # a plane extent outside its buffer
    assert ladder(ctx, [good[0], [desc(small[0]), far]], S) == "badTarget"
    odd = desc(small[1])
    odd.planes[0].offset = 2                                                    # 4-component planes must be 4-byte aligned
    assert ladder(ctx, [good[0], [desc(small[0]), odd]], S) == "badTarget"
    # the same conditions on a source
    for fmt in ("nv12", "y420p"):
        assert ladder(ctx, good, [desc(src[0]), desc(pic(fmt, 96, 96))]) == "badInputData"
    two = desc(src[1])
    two.n_planes = 2
    assert ladder(ctx, good, [desc(src[0]), two]) == "badInputData"
    comps = desc(src[1])
    comps.planes[0].components = 1
    assert ladder(ctx, good, [desc(src[0]), comps]) == "badInputData"
    far = desc(src[1])
    far.planes[0].height = 1 << 20
    assert ladder(ctx, good, [desc(src[0]), far]) == "badInputData"
    # sizes
    assert ladder(ctx, good, [desc(src[0]), desc(pic("bgra", 98, 96))]) == "invalidValue"               # two source sizes
    assert ladder(ctx, [good[0], [desc(small[0]), desc(pic("bgra", 30, 32))]], S) == "invalidValue"    # two sizes in the last rung
    # a refused LAST rung after valid ones: 30:1 trips the 160 KB rule; more than 256 taps
    assert launch_lanczos_refuses(120, 96, 4, 4) and not launch_lanczos_refuses(120, 96, 64, 64) and not launch_lanczos_refuses(120, 96, 32, 32)
    wide = [pic("bgra", 120, 96) for _ in range(2)]
    tiny = [pic("bgra", 4, 4) for _ in range(2)]
    assert ladder(ctx, [good[0], good[1], [desc(g) for g in tiny]], [desc(g) for g in wide]) == "invalidValue"
    assert ladder(ctx, [[desc(g) for g in tiny]], [desc(g) for g in wide]) == "invalidValue"
    assert taps(90, 2) > 256
    tall = [pic("bgra", 8, 90) for _ in range(2)]
    thin = [pic("bgra", 8, 2) for _ in range(2)]
    assert ladder(ctx, [[desc(g) for g in tall], [desc(g) for g in thin]], [desc(g) for g in tall]) == "invalidValue"
    assert counter() == before and others() == others_before, "a refused ladder launched something"
    pic.unchanged("errors")
    # (the pictures the refusals were made from make good ladders: every refusal above is the one it names)
    assert ladder(ctx, good, S) == "success"
    assert ladder(ctx, [good[0]], [desc(g) for g in wide]) == "success"
    assert not launch_lanczos_refuses(64, 64, 4, 4)
    assert ladder(ctx, [[desc(g) for g in tiny]], [desc(g) for g in big]) == "success"
    assert ladder(ctx, [[desc(g) for g in tall]], [desc(g) for g in tall]) == "success"
    assert counter() - before == 4


# ---- 10. foreign layouts -------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def placing(ctx):
    p = Placing(ctx)
    yield p
    p.rec.sweep(ctx)            # every allocation downloaded completely: payload of the targets changed, nothing else, no byte of a source


@pytest.mark.parametrize("fmt,src_layout,dst_layout", [("bgra", "view", "at12p8"), ("rgba", "guarded", "skewed")])
def test_foreign_layouts(ctx, placing, fmt, src_layout, dst_layout):
    """the ladder of (1) on views of larger parents behind guard bands; each allocation is read back whole"""
    n, rungs = 2, tuple(RUNGS)
    srcs, exp = ladder_case(*SRC, rungs, 3)
    gs = [placing.place(fmt, *SRC, [srcs[i]], src_layout) for i in range(n)]
    gd = [[placing.place(fmt, ow, oh, util.alloc_image(fmt, ow, oh, seed=11 + 8 * r + i), dst_layout) for i in range(n)] for r, (ow, oh) in enumerate(rungs)]
    p = placing.rec.placement(gd[0][0]).planes[0]
    assert p.offset % 4 == 0 and p.offset % 16 != 0 and p.pitch % 16 != 0
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosRgbLadder(c, gd, gs))
    assert counter() - before == 2
    for r, (ow, oh) in enumerate(rungs):
        for i in range(n):
            G.assert_same(placing.from_gpu(gd[r][i], fmt, ow, oh), [exp[i][r]], f"{fmt} rung {r}, picture {i}, {src_layout} -> {dst_layout}")


# ---- 11. inside a pass ---------------------------------------------------------------------------------------------------------------------
def test_ladder_inside_a_pass_sees_the_held_composite(ctx):
    cw, ch, sw, sh, rungs = 128, 72, 192, 108, [(64, 36), (96, 54), (24, 14)]
    layer = util.alloc_image("nv12", sw, sh, seed=7)
    u = util.full_canvas_uniforms((cw, ch), (sw, sh))
    canvas = util.alloc_image("bgra", cw, ch, seed=8)
    assert O.run_kernel("img_clear_bgra", canvas) == 0
    assert O.run_kernel("img_nv12_bgra", canvas, layer, u) == 0
    gl = G.to_gpu(ctx, "nv12", sw, sh, layer)
    gc = G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=8))
    gd = [G.to_gpu(ctx, "bgra", ow, oh, util.alloc_image("bgra", ow, oh, seed=9 + r)) for r, (ow, oh) in enumerate(rungs)]

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gc, kernel=K("img_clear_bgra"), blends=False)
        c = sv.runComputeKernel(c, images=[gl], target=gc, kernel=K("img_nv12_bgra"), uniforms=u, blends=True)
        c = sv.scaleLanczosRgbLadder(c, gd, gc)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gc, "bgra", cw, ch), canvas, "the composited canvas")
    for r, (ow, oh) in enumerate(rungs):
        G.assert_same(G.from_gpu(ctx, gd[r], "bgra", ow, oh), [oracle_resize(canvas[0], ow, oh)],
                      f"rung {r}: the rendition of the canvas composited in the same pass")
