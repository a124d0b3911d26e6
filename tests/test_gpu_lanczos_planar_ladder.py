"""chv_scale_lanczos_ladder: every rung of a 4:2:0 encoder ladder — the renditions of one or several NV12 or y420p
pictures of one size as pictures of the same format of up to eight sizes — in one launch per route.  Bit-exact, no tolerance, no case excluded.

The reference is the one tests/test_gpu_lanczos_yuv.py builds (the oracle's 4-channel Lanczos, plane by plane, cached); every ladder is
compared with it AND with the single calls into a second set of targets.  Every target is pre-filled with seeded bytes."""
import ctypes as C
import re
from pathlib import Path

import pytest

import gpuutil as G
import layouts as L
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv
from test_gpu_lanczos_yuv import FORMATS, Placing, case, reference

pytestmark = pytest.mark.gpu

K = sv.defaultComputeKernelFromString
NP = {"nv12": 2, "y420p": 3}

# rungs of a 288 x 144 source (planes of whole 16-byte vectors: the hand-awaited loads): (largest tap count, tap class or route) by
# launch_lanczos_planar's rules
SRC = (288, 144)
RUNGS = {(288, 144): (6, 6), (400, 200): (6, 6),                  # 1:1, an enlargement
         (240, 120): (8, 8),
         (192, 96): (10, 12), (191, 95): (10, 12),                # (odd: floor'd chroma)
         (144, 72): (12, 12), (130, 64): (14, 16), (96, 48): (18, 22), (82, 41): (22, 22),
         (72, 36): (24, "tile"), (101, 37): (24, "tile")}         # past the strips; unequal taps (18 / 24)
WIDE_SRC = (1100, 40)                                             # rows that are no whole vectors: compiler-managed loads; several strips, a partial last one
WIDE = [(550, 20), (733, 27), (367, 13)]                          # 12 taps, 10 taps, 18 / 20 taps that differ between the planes (class 22)
LADDERS = {
    "five_wave": (SRC, [(240, 120), (192, 96), (144, 72)]),                # largest class 12: the five-wave variant
    "four_wave": (SRC, [(192, 96), (130, 64), (82, 41)]),                  # classes 12, 16 and 22 side by side: the four-wave variant
    "mixed": (SRC, [(144, 72), (72, 36), (101, 37), (96, 48)]),            # two launches
    "tile_only": (SRC, [(72, 36)]),
    "one_rung": (SRC, [(192, 96)]),
    "eight": (SRC, [(288, 144), (400, 200), (191, 95), (144, 72), (191, 95), (82, 41), (72, 36), (101, 37)]),      # a size twice, the 1:1 rung
    "wide": (WIDE_SRC, WIDE),
}
MIXED = LADDERS["mixed"]


def counter():
    return cv.get_counter("lanczos_planar_ladder_launches")


def references(fmt, src_size, sizes, n):
    """(source planes, exp[r][i]) from the shared, cached reference: sources 900 .. 900 + n - 1 of that size"""
    iw, ih = src_size
    srcs, exps = [None] * n, [[None] * n for _ in sizes]
    for r, (w, h) in enumerate(sizes):
        for i in range(n):
            srcs[i], exps[r][i] = case(fmt, iw, ih, w, h, 900 + i)
    return srcs, exps


def fresh_targets(ctx, fmt, sizes, n, seed, place=None):
    """rungs[r][i], each pre-filled with seeded bytes"""
    put = place or (lambda f, w, h, planes: G.to_gpu(ctx, f, w, h, planes))
    return [[put(fmt, w, h, util.alloc_image(fmt, w, h, seed=seed + 16 * r + i)) for i in range(n)] for r, (w, h) in enumerate(sizes)]


def check_rungs(ctx, fmt, sizes, rungs, exps, what, singles=None, read=None):
    read = read or (lambda sample, f, w, h: G.from_gpu(ctx, sample, f, w, h))
    for r, (w, h) in enumerate(sizes):
        for i, gd in enumerate(rungs[r]):
            got = read(gd, fmt, w, h)
            G.assert_same(got, exps[r][i], f"{what}: rung {r} ({w}x{h}) of source {i} against the reference")
            if singles:
                G.assert_same(got, read(singles[r][i], fmt, w, h), f"{what}: rung {r} ({w}x{h}) of source {i} against the single call")


# ---- 1. the ladders ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(LADDERS))
def test_ladder_equals_the_single_calls_and_the_reference(ctx, name, fmt, n):
    src_size, sizes = LADDERS[name]
    srcs, exps = references(fmt, src_size, sizes, n)
    gs = [G.to_gpu(ctx, fmt, *src_size, s) for s in srcs]
    rungs, singles = fresh_targets(ctx, fmt, sizes, n, 3), fresh_targets(ctx, fmt, sizes, n, 1003)
    sv.usingContext(ctx, lambda c: sv.scaleLanczosLadder(c, rungs, gs if n > 1 else gs[0]))
    for r in range(len(sizes)):
        for i in range(n):
            sv.usingContext(ctx, lambda c: sv.scaleLanczos(c, singles[r][i], gs[i]))
    check_rungs(ctx, fmt, sizes, rungs, exps, f"{name} ladder, {fmt}, {n} source(s)", singles)


def test_every_rung_of_the_table_is_in_a_ladder():
    assert {s for src, sizes in LADDERS.values() if src == SRC for s in sizes} == set(RUNGS)


# ---- 2. launches -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,launches", [("five_wave", 1), ("four_wave", 1), ("tile_only", 1), ("mixed", 2), ("eight", 2)])
def test_launch_counter(ctx, name, launches):
    """the strip rungs leave in one launch, the tile rungs in one more: never more than two, whatever the rungs"""
    src_size, sizes = LADDERS[name]
    assert src_size == SRC and launches == len({RUNGS[s][1] == "tile" for s in sizes})
    srcs, exps = references("nv12", src_size, sizes, 3)
    gs = [G.to_gpu(ctx, "nv12", *src_size, s) for s in srcs]
    rungs = fresh_targets(ctx, "nv12", sizes, 3, 5)
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosLadder(c, rungs, gs))
    assert counter() - before == launches
    check_rungs(ctx, "nv12", sizes, rungs, exps, f"{name} ladder under the counter")


def header_chunk(n_rungs, planes):
    """CHV_PLANAR_LADDER_CHUNK of include/chipvideo.h, from the header's own text and numbers"""
    text = (Path(__file__).resolve().parents[1] / "include" / "chipvideo.h").read_text()
    slot = int(re.search(r"#define CHV_LADDER_SLOT_BYTES (\d+)", text).group(1))
    plane = int(re.search(r"#define CHV_LADDER_PLANE_BYTES (\d+)", text).group(1))
    assert "#define CHV_PLANAR_LADDER_CHUNK(n_rungs, planes) (CHV_LADDER_SLOT_BYTES / ((((n_rungs) + 1) * (planes)) * CHV_LADDER_PLANE_BYTES))" in text
    return slot // (((n_rungs + 1) * planes) * plane)


# ---- 3. the chunk boundary ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_chunk_boundary(ctx, fmt):
    """one chunk plus one picture, a strip rung and a tile rung: two chunks of two launches, all rungs of a picture in one chunk"""
    src_size, sizes = (40, 24), [(20, 12), (10, 6)]
    n = header_chunk(len(sizes), NP[fmt]) + 1
    assert n > 2
    srcs, exps = references(fmt, src_size, sizes, n)
    gs = [G.to_gpu(ctx, fmt, *src_size, s) for s in srcs]
    rungs, singles = fresh_targets(ctx, fmt, sizes, n, 7), fresh_targets(ctx, fmt, sizes, n, 2007)
    before = counter()
    sv.usingContext(ctx, lambda c: sv.scaleLanczosLadder(c, rungs, gs))
    assert counter() - before == 4
    for r in range(len(sizes)):
        sv.usingContext(ctx, lambda c: sv.LanczosBatch(list(zip(singles[r], gs))).run(c))
    check_rungs(ctx, fmt, sizes, rungs, exps, f"{n} pictures of {fmt}", singles)


# ---- 4. the replayable object ------------------------------------------------------------------------------------------------------------
def test_the_ladder_object_replays(ctx):
    src_size, sizes = MIXED
    srcs, exps = references("y420p", src_size, sizes, 2)
    gs = [G.to_gpu(ctx, "y420p", *src_size, s) for s in srcs]
    rungs = fresh_targets(ctx, "y420p", sizes, 2, 9)
    ladder = sv.LanczosLadder(rungs, gs)
    before = counter()
    sv.usingContext(ctx, lambda c: ladder.run(c))
    check_rungs(ctx, "y420p", sizes, rungs, exps, "first run")
    sv.usingContext(ctx, lambda c: ladder.run(c))
    assert counter() - before == 4
    check_rungs(ctx, "y420p", sizes, rungs, exps, "second run")


# ---- 5. foreign layouts ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def placing(ctx):
    p = Placing(ctx)
    yield p
    p.rec.sweep(ctx)            # every allocation downloaded completely: payload of the targets changed, nothing else, no byte of a source


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("src_layout,dst_layout", [(l, l) for l in L.LAYOUTS] + [("guarded", "skewed"), ("skewed", "guarded"), ("view", "tight"),
                                                   ("guarded", "at1p3"), ("guarded", "at4p4"), ("tight", "at2p6")])
def test_foreign_layouts(ctx, placing, fmt, src_layout, dst_layout):
    """the kernels index planes by rung, picture and plane: every allocation is read back whole, so a wrong index shows as a changed guard
    byte, a changed source or an unchanged target"""
    src_size, sizes = MIXED
    srcs, exps = references(fmt, src_size, sizes, 2)
    gs = [placing.place(fmt, *src_size, s, src_layout) for s in srcs]
    rungs = fresh_targets(ctx, fmt, sizes, 2, 13, place=lambda f, w, h, planes: placing.place(f, w, h, planes, dst_layout))
    sv.usingContext(ctx, lambda c: sv.scaleLanczosLadder(c, rungs, gs))
    check_rungs(ctx, fmt, sizes, rungs, exps, f"mixed ladder, sources on {src_layout}, targets on {dst_layout}", read=placing.from_gpu)


# ---- 6. inside a pass --------------------------------------------------------------------------------------------------------------------
def test_ladder_inside_a_pass_sees_the_held_composite(ctx):
    cw, ch, sizes = 128, 72, [(96, 54), (64, 36), (32, 18)]       # (the last one: 24 taps, the tile route)
    layer = util.alloc_image("bgra", 40, 30, seed=7)
    u = util.make_uniforms((cw, ch), rect=(10, 6, 60, 40), border=(2, 2, 2, 2), fill=(0.2, 0.6, 0.3, 0.7), opacity=0.8, in_size=(40, 30))
    canvas = util.alloc_image("nv12", cw, ch, seed=8)
    assert O.run_kernel("img_clear_nv12", canvas) == 0
    assert O.run_kernel("img_bgra_nv12", canvas, layer, u) == 0
    exps = [[reference("nv12", canvas, cw, ch, w, h)] for w, h in sizes]
    gl = G.to_gpu(ctx, "bgra", 40, 30, layer)
    gc = G.to_gpu(ctx, "nv12", cw, ch, util.alloc_image("nv12", cw, ch, seed=8))
    rungs = fresh_targets(ctx, "nv12", sizes, 1, 15)

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gc, kernel=K("img_clear_nv12"), blends=False)
        c = sv.runComputeKernel(c, images=[gl], target=gc, kernel=K("img_bgra_nv12"), uniforms=u, blends=True)
        c = sv.scaleLanczosLadder(c, rungs, gc)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gc, "nv12", cw, ch), canvas, "the composited canvas")
    check_rungs(ctx, "nv12", sizes, rungs, exps, "the ladder of the canvas composited in the same pass")


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------
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
    rc = cv.load().chv_scale_lanczos_ladder(ctx.handle, d, len(rung_descs) if n_rungs is None else n_rungs, s, len(src_descs) if n is None else n)
    if rc == 0:
        return "success"
    with pytest.raises(sv.ComputeError) as e:
        cv.check(rc)
    return e.value.case


def test_errors_leave_every_rung_unchanged(ctx):
    pic, desc = Pictures(ctx), sv._image_desc
    src = [pic("nv12", 64, 36), pic("nv12", 64, 36)]
    nv = [[pic("nv12", 32, 18), pic("nv12", 32, 18)], [pic("nv12", 16, 10), pic("nv12", 16, 10)]]
    yp = [pic("y420p", 16, 10), pic("y420p", 16, 10)]
    ysrc = [pic("y420p", 64, 36), pic("y420p", 64, 36)]
    D = lambda rows: [[desc(g) for g in row] for row in rows]      # noqa: E731
    S = lambda row: [desc(g) for g in row]                         # noqa: E731
    nine = [[pic("nv12", 8 + 2 * r, 6)] for r in range(9)]
    assert status(ctx, D(nine), S(src[:1])) == "invalidValue"                                   # n_rungs = 9
    assert status(ctx, D(nv), S(src), n_rungs=-1) == "invalidValue"
    assert status(ctx, D(nv), S(src), n=-1) == "invalidValue"
    lib = cv.load()
    with pytest.raises(sv.ComputeError) as e:                                                   # a NULL list with non-zero counts
        cv.check(lib.chv_scale_lanczos_ladder(ctx.handle, None, 1, C.byref(desc(src[0])), 1))
    assert e.value.case == "invalidValue"
    with pytest.raises(sv.ComputeError) as e:
        cv.check(lib.chv_scale_lanczos_ladder(ctx.handle, C.byref(desc(nv[0][0])), 1, None, 1))
    assert e.value.case == "invalidValue"
    assert status(ctx, D([[pic("bgra", 32, 18)]]), S([pic("bgra", 64, 36)])) == "badTarget"    # a BGRA dsts[0]: no 4-component family here
    one = D(nv)
    one[0][0].n_planes = 1                                                                      # an nv12 dsts[0] with one plane
    assert status(ctx, one, S(src)) == "badTarget"
    assert status(ctx, D([nv[0], yp]), S(src)) == "invalidValue"                                # targets that differ in format
    assert status(ctx, D([yp, nv[0]]), S(ysrc)) == "invalidValue"
    assert status(ctx, D(nv), S([src[0], ysrc[1]])) == "invalidValue"                           # a y420p source among NV12 sources
    assert status(ctx, D(nv), S(ysrc)) == "badInputData"                                        # y420p sources for NV12 targets
    assert status(ctx, D([nv[0], [nv[1][0], nv[0][1]]]), S(src)) == "invalidValue"              # two sizes inside a rung
    assert status(ctx, D(nv), S([src[0], pic("nv12", 80, 36)])) == "invalidValue"               # two source sizes
    far = D(nv)
    far[1][1].planes[1].height = 1 << 20                                                        # a bad chroma plane in the last rung: its extent leaves its buffer
    assert status(ctx, far, S(src)) == "badTarget"
    away = S(src)
    away[1].planes[1].offset = away[1].planes[1].offset + (1 << 30)                             # a source plane that fails a plane check
    assert status(ctx, D(nv), away) == "badInputData"
    big = pic("nv12", 96, 96)                                                                   # the LAST rung is 24:1: the 160 KB rule
    first, tiny = pic("nv12", 48, 48), pic("nv12", 4, 4)
    assert status(ctx, D([[first], [tiny]]), S([big])) == "invalidValue"
    pic.unchanged("errors")
    # (the lists the refusals were made from are good ladders: every refusal above is the one it names)
    assert status(ctx, D(nv), S(src)) == "success"
    assert status(ctx, D([yp]), S(ysrc)) == "success"
    assert status(ctx, D([[first]]), S([big])) == "success"


# ---- 8. empty ladders --------------------------------------------------------------------------------------------------------------------
def test_empty_ladders_are_noops(ctx):
    pic, desc = Pictures(ctx), sv._image_desc
    src, dst = pic("nv12", 64, 36), pic("nv12", 32, 18)
    before = counter()
    assert status(ctx, [[desc(dst)]], [desc(src)], n_rungs=0) == "success"
    assert status(ctx, [[desc(dst)]], [desc(src)], n=0) == "success"
    lib = cv.load()
    cv.check(lib.chv_scale_lanczos_ladder(ctx.handle, None, 0, None, 0))
    cv.check(lib.chv_scale_lanczos_ladder(ctx.handle, None, 0, None, 3))
    cv.check(lib.chv_scale_lanczos_ladder(ctx.handle, None, 3, None, 0))
    assert sv.scaleLanczosLadder(ctx, [], []) is ctx
    assert counter() == before
    pic.unchanged("an empty ladder")
