"""Every kernel route on FOREIGN plane layouts with guard bands (tests/layouts.py).

The rest of the GPU suite uploads every picture through uploadComputePicture — a fresh allocation, offset 0, 128-byte pitches — and crops what
it downloads to the payload.  Here the same seeded generators run with their pictures placed the other ways the C ABI allows (DESIGN.md
section 2): behind guards, as sub-rectangles of larger parents, packed to 16 bytes, tight, and skewed off every vector boundary.  Each test
holds the result against the oracle bit for bit as before, and at teardown every allocation is downloaded completely: a launch may have
written payload bytes of its target's planes and nothing else — not its pitch padding, not the bytes in front of it or behind its last row,
not a neighbour's pixels, not a byte of a source.

Routes: on `guarded`, `view` and `packed16` every batch must be launched through the kernel the identical ticks take on the plain layout
(both are built, the names compared); on `tight` and `skewed` no vector route may appear whose predicate requires a 16-byte aligned plane
that the placement did not give it.  test_zz_routes_seen prints the kernel names seen per layout (-s)."""
import zlib

import numpy as np
import pytest

import gpuutil as G
import layouts as L
import scenarios as S
import test_gpu_fastpath as FP
import test_gpu_fuzz as FZ
import test_gpu_geom_store as GS
import test_gpu_mixpath as MIX
import test_gpu_parity as PAR
import test_gpu_yuvstream as YST
import test_gpu_yuvwave as YWV
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv

pytestmark = pytest.mark.gpu

ALL_LAYER = S.LAYER_KERNELS_REF + S.LAYER_KERNELS_OWN + S.LAYER_KERNELS_INT
ROUTES_SEEN = {}             # layout -> {kernel name: batches}
K = sv.defaultComputeKernelFromString


class Placing:
    """gpuutil.to_gpu / from_gpu / make_batch replaced for one test: pictures are placed on `name`, every batch's route is checked"""

    def __init__(self, ctx, monkeypatch, name):
        self.ctx, self.name, self.rec, self.n = ctx, name, L.Recorder(), 0
        self.plain_to, self.plain_from, self.plain_make = G.to_gpu, G.from_gpu, G.make_batch
        self.names = []
        monkeypatch.setattr(G, "to_gpu", self.to_gpu)
        monkeypatch.setattr(G, "from_gpu", self.from_gpu)
        monkeypatch.setattr(G, "make_batch", self.make_batch)

    def place(self, fmt, w, h, planes, layout=None, **kw):
        layout = layout or self.name
        self.n += 1
        sample = L.place(self.ctx, fmt, w, h, planes, layout, seed=(zlib.crc32(layout.encode()) & 0xFFFF) * 4096 + self.n, recorder=self.rec, **kw)
        if layout == "skewed":
            assert any(p.offset % 16 or p.pitch % 16 for p in self.rec.placement(sample).planes), "a skewed picture with every plane on vector boundaries"
        return sample

    def to_gpu(self, ctx, fmt, w, h, planes, **kw):
        assert ctx is self.ctx
        return self.place(fmt, w, h, planes, **kw)

    def from_gpu(self, ctx, sample, fmt, w, h):
        return L.from_gpu(self.rec, self.plain_from, ctx, sample, fmt, w, h)

    def twin(self, sample, cache):
        """the same picture on the plain layout (uploadComputePicture)"""
        if self.rec.placement(sample) is None:
            return sample
        key = id(sample.imageBuffer().computeTextures[0])
        if key not in cache:
            cache[key] = self.plain_to(self.ctx, *self.rec.host_copy(sample))
        return cache[key]

    def make_batch(self, ctx, ticks):
        h, name, keep = self.plain_make(ctx, ticks)
        try:
            placements = [self.rec.placement(t) for t, _, _ in ticks] + [self.rec.placement(s) for _, _, ls in ticks for _, s, _, _ in ls]
            kinds = {p.layout for p in placements if p is not None}
            if kinds and kinds <= set(L.SAME_ROUTE):
                cache = {}
                plain = [(self.twin(t, cache), clear, [(k, self.twin(s, cache), u, csc) for k, s, u, csc in ls]) for t, clear, ls in ticks]
                h2, name2, keep2 = self.plain_make(ctx, plain)
                G.destroy_batch(h2)
                assert name == name2, f"layout {sorted(kinds)}: launched through {name}, the same ticks on the plain layout through {name2}"
            else:
                bad = L.route_violations(name, self.rec, ticks)
                assert not bad, f"layout {sorted(kinds)}: {bad} launched although a plane its predicate wants on 16-byte boundaries is not"
        except BaseException:
            G.destroy_batch(h)
            raise
        seen = ROUTES_SEEN.setdefault(self.name, {})
        seen[name] = seen.get(name, 0) + 1
        self.names.append(name)
        return h, name, keep

    def sweep(self):
        return self.rec.sweep(self.ctx)


@pytest.fixture(params=L.LAYOUTS)
def layout(request, ctx, monkeypatch):
    p = Placing(ctx, monkeypatch, request.param)
    yield p
    p.sweep()


@pytest.fixture
def guarded(ctx, monkeypatch):
    """sources (and whatever else the generators upload) on the `guarded` layout; the tests place their own targets"""
    p = Placing(ctx, monkeypatch, "guarded")
    yield p
    p.sweep()


def _run_ticks(ctx, ticks, exps, gds, fmt, what, lone=False):
    """a batch (or lone ticks through chv_composite) of generator output -> the kernel name; every canvas against the oracle's"""
    name = "chv_composite"
    if lone:
        for gd, clear, layers in ticks:
            sv.usingContext(ctx, lambda c: sv.compositeTick(c, gd, layers, clear))
    else:
        h, name, keep = G.make_batch(ctx, ticks)
        G.run_batch(ctx, h)
        G.destroy_batch(h)
    for i, ((gd, cw, ch), exp) in enumerate(zip(gds, exps)):
        G.assert_same(G.from_gpu(ctx, gd, fmt, cw, ch), exp, f"{what} tick {i} ({cw}x{ch}) via {name}")
    return name


# ---- single launches --------------------------------------------------------------------------------------------------------------
def _geometry(kernel, geometry):
    if geometry in S.SCENARIOS:
        cw, ch, iw, ih, _ = S.SCENARIOS[geometry]
        return cw, ch, iw, ih, S.uniforms_for(geometry), 0
    rng = np.random.default_rng(1040 + int(geometry[-1]) + 16 * ALL_LAYER.index(kernel))          # (test_gpu_fuzz.py stops at 1039)
    cw, ch, iw, ih, kw = FZ._random_case(rng)
    s, d = G.kernel_formats(kernel)
    if s in ("nv12", "y420p"):
        iw, ih = max(iw, 2), max(ih, 2)
    return cw, ch, iw, ih, util.make_uniforms((cw, ch), in_size=(iw, ih), **kw), int(rng.integers(0, 4))


@pytest.mark.parametrize("geometry", list(S.SCENARIOS) + ["random0", "random1"])
@pytest.mark.parametrize("kernel", ALL_LAYER)
def test_single_launches(ctx, layout, kernel, geometry):
    """chv_run_kernel onto a seeded canvas, chv_composite onto a cleared one"""
    cw, ch, iw, ih, u, csc = _geometry(kernel, geometry)
    seed = (zlib.crc32(f"layouts/{kernel}/{geometry}".encode()) & 0xFFFF) + 1
    for clear_first in (False, True):
        got, exp = G.run_both(ctx, kernel, cw, ch, iw, ih, u, seed + clear_first, csc=csc, clear_first=clear_first)
        G.assert_same(got, exp, f"{kernel}/{geometry} on {layout.name}, {'chv_composite' if clear_first else 'chv_run_kernel'}")


CLEAR_SIZES = [("bgra", w, h) for w in (1, 3, 5, 17, 130, 132) for h in (1, 2, 9)] + \
              [(f, w, h) for f in ("nv12", "y420p") for w, h in ((130, 2), (132, 2), (7, 5))]


@pytest.mark.parametrize("fmt,w,h", CLEAR_SIZES)
def test_clears(ctx, layout, fmt, w, h):
    """the fast clear's vector body and scalar tail; 7 x 5 on 4:2:0: the general kernel"""
    canvas0 = util.alloc_image(fmt, w, h, seed=5 + w)
    exp = util.copy_image(canvas0)
    assert O.run_kernel(f"img_clear_{fmt}", exp) == 0
    g = G.to_gpu(ctx, fmt, w, h, canvas0)
    sv.usingContext(ctx, lambda c: sv.runComputeKernel(c, images=[], target=g, kernel=K(f"img_clear_{fmt}")))
    G.assert_same(G.from_gpu(ctx, g, fmt, w, h), exp, f"clear {fmt} {w}x{h} on {layout.name}")


# ---- forced routes in batches: six seeds each, continuing where tests/test_gpu_fuzz.py stops ---------------------------------------
@pytest.mark.parametrize("seed", range(90, 96))
def test_bgra_stream_route(ctx, switch, layout, seed):
    switch("CHV_BGRA_PATH", "stream")
    ticks, exps, gds = MIX._random_stream_ticks(ctx, seed)
    _run_ticks(ctx, ticks, exps, gds, "bgra", f"stream seed {seed} on {layout.name}")


@pytest.mark.parametrize("rows", ["8", "16"])
@pytest.mark.parametrize("seed", range(126, 132))
def test_strip_routes(ctx, switch, layout, rows, seed):
    """tick_bgra_wave, and tick_yuv_wave on NV12 (even seeds) and y420p (odd seeds) canvases"""
    switch("CHV_BGRA_PATH", "wave")
    switch("CHV_YUV_STREAM", "0")
    switch("CHV_WAVE_ROWS", rows)
    MIX.test_random_mixed_ticks(ctx, MIX.WAVE, seed)
    YWV.test_random_yuv_ticks(ctx, rows, seed)


@pytest.mark.parametrize("seed", range(40, 46))
def test_rgb_only_strips_with_and_without_dma_staging(ctx, switch, layout, seed):
    switch("CHV_BGRA_PATH", "wave")
    for dma in ("0", None):
        switch("CHV_WAVE_DMA", dma)
        ticks, exps, gds = MIX._random_rgb_only_ticks(ctx, seed)
        _run_ticks(ctx, ticks, exps, gds, "bgra", f"RGB-only seed {seed}, CHV_WAVE_DMA={dma}, on {layout.name}")


@pytest.mark.parametrize("seed", range(252, 258))
def test_yuv_stream_route(ctx, switch, layout, seed):
    """CHV_YUV_STREAM=force: float and integer-matrix RGB layers"""
    switch("CHV_YUV_STREAM", "force")
    for integer in (False, True):
        rng = np.random.default_rng(21000 + seed + 100 * integer)
        d = "nv12" if seed % 2 == 0 else "y420p"
        built = [YST.build_random(ctx, rng, d, integer) for _ in range(3)]
        _run_ticks(ctx, [(b[0], True, b[3]) for b in built], [b[4] for b in built], [(b[0], b[1], b[2]) for b in built], d,
                   f"yuv stream seed {seed} int {integer} on {layout.name}")


@pytest.mark.parametrize("seed", range(60, 66))
def test_general_route(ctx, switch, layout, seed):
    switch("CHV_FORCE_GENERAL", "1")
    MIX.test_random_mixed_ticks(ctx, None, seed)
    YWV.test_random_yuv_ticks(ctx, "8", seed)


@pytest.mark.parametrize("rows", ["16", "32"])
@pytest.mark.parametrize("seed", range(24, 30))
def test_tiled_routes(ctx, switch, layout, rows, seed):
    switch("CHV_BGRA_PATH", "tiled")
    FP.test_random_axis_aligned_yuv_bgra_ticks(ctx, switch, seed, rows)


@pytest.mark.parametrize("case", ["mixed_scale", "noclear"])
def test_rgb_tiled_cases(ctx, layout, case):
    cw, ch, clear, specs = FP.RGB_CASES[case]
    MIX.run_tick_case(ctx, cw, ch, clear, specs, seed=61, expect=None)


# ---- skewed destinations beside aligned sources ------------------------------------------------------------------------------------
DST4 = ["at4p4", "at8p4", "at12p4"]                                     # what the streaming kernels ask of a destination: 4-byte alignment
DST_ANY = DST4 + ["at1p1", "at3p2", "at6p0", "at5p3", "at2p2"]           # the 4:2:0 strip kernel asks nothing: odd addresses, pitch = 0, 2, 1, 3 mod 4


def _retarget(placing, ticks, gds, fmt, layouts, seed):
    """every tick's target replaced by a newly placed one (a cleared tick does not read its canvas)"""
    out_ticks, out_gds = [], []
    for t, ((gd, clear, layers), (_, cw, ch)) in enumerate(zip(ticks, gds)):
        assert clear
        new = placing.place(fmt, cw, ch, util.alloc_image(fmt, cw, ch, seed=900 + seed + t), layout=layouts[(seed + t) % len(layouts)])
        out_ticks.append((new, True, layers))
        out_gds.append((new, cw, ch))
    return out_ticks, out_gds


@pytest.mark.parametrize("lone", [False, True], ids=["batch", "lone"])
@pytest.mark.parametrize("seed", range(96, 102))
def test_skewed_destination_bgra_stream(ctx, switch, guarded, seed, lone):
    switch("CHV_BGRA_PATH", "stream")
    ticks, exps, gds = MIX._random_stream_ticks(ctx, seed)
    h, plain_name, keep = guarded.plain_make(ctx, ticks)
    G.destroy_batch(h)
    ticks, gds = _retarget(guarded, ticks, gds, "bgra", DST4, seed)
    name = _run_ticks(ctx, ticks, exps, gds, "bgra", f"stream seed {seed}, skewed destination", lone=lone)
    if not lone and plain_name == MIX.STREAM:            # (a rectangle wider than 1.7 source texels per pixel never was the streaming kernel's)
        assert name == MIX.STREAM, name


@pytest.mark.parametrize("lone", [False, True], ids=["batch", "lone"])
@pytest.mark.parametrize("seed", range(258, 264))
def test_skewed_destination_yuv_stream(ctx, switch, guarded, seed, lone):
    switch("CHV_YUV_STREAM", "force")
    rng = np.random.default_rng(21000 + seed)
    d = "nv12" if seed % 2 == 0 else "y420p"
    built = [YST.build_random(ctx, rng, d, seed % 3 == 0) for _ in range(3)]
    ticks, gds = _retarget(guarded, [(b[0], True, b[3]) for b in built], [(b[0], b[1], b[2]) for b in built], d, DST4, seed)
    name = _run_ticks(ctx, ticks, [b[4] for b in built], gds, d, f"yuv stream seed {seed}, skewed destination", lone=lone)
    if not lone:
        assert name == f"tick_yuv_stream<{d}>", name


@pytest.mark.parametrize("lone", [False, True], ids=["batch", "lone"])
@pytest.mark.parametrize("rows", ["8", "16"])
@pytest.mark.parametrize("seed", range(132, 138))
def test_skewed_destination_yuv_strips(ctx, switch, guarded, rows, seed, lone):
    """tick_yuv_wave picks 4-byte / 8-byte or byte stores per strip at run time from the destination's address and pitch: canvases of width
    0 and 2 mod 4 at addresses and pitches of every residue"""
    switch("CHV_YUV_STREAM", "0")
    switch("CHV_WAVE_ROWS", rows)
    d, _, ticks, exps, gds = YWV._random_yuv_ticks(ctx, seed, clear=True)
    h, plain_name, keep = guarded.plain_make(ctx, ticks)
    G.destroy_batch(h)
    ticks, gds = _retarget(guarded, ticks, gds, d, DST_ANY, seed)
    name = _run_ticks(ctx, ticks, exps, gds, d, f"yuv strips seed {seed}, skewed destination", lone=lone)
    if not lone and plain_name == f"tick_yuv_wave<{d}>":       # (strong downscales of 4-byte texels exceed the LDS budget on any layout)
        assert name == f"tick_yuv_wave<{d}>", name


def test_skewed_destinations_reach_the_strip_kernel(ctx, switch, guarded):
    """the fixed case behind the seeds above: a mixer tick on canvases of width 0 and 2 mod 4 with pitch 0, 2 and 1 mod 4 must stay tick_yuv_wave"""
    switch("CHV_YUV_STREAM", "0")
    for d in ("nv12", "y420p"):
        for cw, lay in ((136, "at4p4"), (134, "at2p2"), (136, "at1p1"), (134, "at7p5"), (136, "at3p2"), (134, "at6p0")):
            ch = 40
            specs = [(f"img_{d}_{d}", 160, 48, dict()), (f"img_bgra_{d}", 64, 36, dict(rect=(9, 3, 90, 30), opacity=0.7))]
            exp = util.alloc_image(d, cw, ch, seed=3)
            assert O.run_kernel(f"img_clear_{d}", exp) == 0
            layers = []
            for i, (k, sw, sh, kw) in enumerate(specs):
                u = util.make_uniforms((cw, ch), in_size=(sw, sh), **kw)
                src = util.alloc_image(k.split("_")[1], sw, sh, seed=50 + i)
                assert O.run_kernel(k, exp, src, u) == 0
                layers.append((K(k), G.to_gpu(ctx, k.split("_")[1], sw, sh, src), u, 0))
            gd = guarded.place(d, cw, ch, util.alloc_image(d, cw, ch, seed=4), layout=lay)
            assert (cw % 4, guarded.rec.placement(gd).planes[0].pitch % 4) in ((0, 0), (2, 2), (0, 1), (2, 1), (0, 2), (2, 0))
            name = _run_ticks(ctx, [(gd, True, layers)], [exp], [(gd, cw, ch)], d, f"{d} {cw}x{ch} on {lay}")
            assert name == f"tick_yuv_wave<{d}>", (name, lay)


# ---- lone ticks: descriptors as kernel arguments, scenes served from the geometry store ---------------------------------------------
@pytest.mark.parametrize("seed", range(118, 124))
def test_lone_stream_ticks(ctx, layout, seed):
    ticks, exps, gds = MIX._random_stream_ticks(ctx, seed, nl_low=1)
    _run_ticks(ctx, ticks, exps, gds, "bgra", f"lone stream seed {seed} on {layout.name}", lone=True)


@pytest.mark.parametrize("seed", range(24, 30))
def test_lone_yuv_stream_ticks(ctx, switch, layout, seed):
    switch("CHV_YUV_STREAM", "force")
    YST.test_random_lone_yuv_stream_ticks(ctx, seed)


@pytest.mark.parametrize("dst", ["bgra", "nv12", "y420p"])
def test_scene_ticked_four_times(ctx, switch, layout, dst):
    """a scene is served from the geometry store on its third sighting — the five layouts of this test tick ONE scene, so tables built behind
    one layout serve the others; CHV_DESC=device once"""
    GS._force_strips(switch, dst)
    switch("CHV_GEOM_CACHE", None)
    cw, ch = 240, 136
    scene = GS._scene(dst, cw, ch, 288, 168)
    for desc in (None, "device"):
        switch("CHV_DESC", desc)
        for t in range(4 if desc is None else 1):
            gd, layers, exp, keep = GS._tick(ctx, dst, cw, ch, scene, 2100 + t)
            sv.usingContext(ctx, lambda c: sv.compositeTick(c, gd, layers, True))
            G.assert_same(G.from_gpu(ctx, gd, dst, cw, ch), exp, f"{dst} scene tick {t} on {layout.name}, CHV_DESC={desc}")


@pytest.mark.parametrize("dst", ["bgra", "nv12", "y420p"])
def test_held_pass(ctx, switch, layout, dst):
    GS._force_strips(switch, dst)
    cw, ch = 240, 136
    gd, layers, exp, keep = GS._tick(ctx, dst, cw, ch, GS._scene(dst, cw, ch, 288, 168), 2200)

    def seq(c):
        c = sv.beginComputePass(c)
        c = sv.runComputeKernel(c, images=[], target=gd, kernel=K(f"img_clear_{dst}"), blends=False)
        for k, g, u, csc in layers:
            c = sv.runComputeKernel(c, images=[g], target=gd, kernel=k, uniforms=u, blends=True, colorspace=csc)
        return sv.endComputePass(c, True)
    sv.usingContext(ctx, seq)
    G.assert_same(G.from_gpu(ctx, gd, dst, cw, ch), exp, f"held pass, {dst} on {layout.name}")


# ---- one scene, changing layouts: the store's key holds neither address nor pitch ---------------------------------------------------
def _changing(dst):
    """(layout of the sources, layout of the canvas) tick by tick"""
    skew_dst = "at4p4" if dst == "bgra" else "at1p1"
    return [("guarded", "guarded"), ("view", "view"), ("packed16", "packed16"), ("guarded", skew_dst), ("skewed", "skewed"),
            ("guarded", "guarded"), ("view", "view"), ("packed16", "packed16")]


def _strip_route(dst, src_layout, dst_layout):
    """does the scene stay on the strip kernel?  Its layers are all staged: their sources must be on vector boundaries, and a BGRA canvas too"""
    return src_layout in L.SAME_ROUTE and (dst != "bgra" or dst_layout in L.SAME_ROUTE)


def _placed_tick(placing, dst, cw, ch, scene, seed, src_layout, dst_layout):
    placing.name = src_layout
    gd0, layers, exp, keep = GS._tick(placing.ctx, dst, cw, ch, scene, seed)
    gd = placing.place(dst, cw, ch, util.alloc_image(dst, cw, ch, seed=seed), layout=dst_layout)
    return gd, layers, exp


@pytest.mark.parametrize("dst", ["bgra", "nv12", "y420p"])
def test_one_scene_changing_layouts_lone(ctx, switch, monkeypatch, dst):
    GS._force_strips(switch, dst)
    switch("CHV_GEOM_CACHE", None)
    placing = Placing(ctx, monkeypatch, "guarded")
    cw, ch = 496, 272                                   # (a canvas size of this test's own: the store is the process's)
    scene = GS._scene(dst, cw, ch, 400, 240)
    b0, p0 = cv.get_counter("geom_store_builds"), cv.get_counter("geom_store_patched")
    on_strips = 0
    for t, (sl, dl) in enumerate(_changing(dst)):
        gd, layers, exp = _placed_tick(placing, dst, cw, ch, scene, 3100 + t, sl, dl)
        sv.usingContext(ctx, lambda c: sv.compositeTick(c, gd, layers, True))
        G.assert_same(G.from_gpu(ctx, gd, dst, cw, ch), exp, f"{dst} tick {t}: sources {sl}, canvas {dl}")
        placing.sweep()
        on_strips += _strip_route(dst, sl, dl)
    assert cv.get_counter("geom_store_builds") == b0 + 1
    # first sighting in place, second builds, every later strip tick is served
    assert cv.get_counter("geom_store_patched") == p0 + on_strips - 2, (on_strips, cv.get_counter("geom_store_patched") - p0)


@pytest.mark.parametrize("dst", ["bgra", "nv12", "y420p"])
def test_one_scene_changing_layouts_batches(ctx, switch, monkeypatch, dst):
    """a batch per layout, run once and destroyed"""
    GS._force_strips(switch, dst)
    switch("CHV_GEOM_CACHE", None)
    placing = Placing(ctx, monkeypatch, "guarded")
    cw, ch = 528, 288
    scene = GS._scene(dst, cw, ch, 400, 240)
    b0 = cv.get_counter("geom_store_builds")
    for t, (sl, dl) in enumerate(_changing(dst)):
        made = [_placed_tick(placing, dst, cw, ch, scene, 3300 + 10 * t + i, sl, dl) for i in range(2)]
        name = _run_ticks(ctx, [(gd, True, layers) for gd, layers, exp in made], [exp for gd, layers, exp in made],
                          [(gd, cw, ch) for gd, layers, exp in made], dst, f"{dst} batch {t}: sources {sl}, canvas {dl}")
        assert ("wave" in name) == _strip_route(dst, sl, dl), (name, sl, dl)
        placing.sweep()
    assert cv.get_counter("geom_store_builds") == b0 + 1


# ---- Lanczos-3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(100, 106))
def test_lanczos_random(ctx, layout, seed):
    PAR.test_lanczos_random_geometries(ctx, seed)


@pytest.mark.parametrize("iw,ih,ow,oh", [(3, 5, 7, 9), (257, 131, 129, 66), (146, 20, 73, 10)])
def test_lanczos_paths(ctx, layout, iw, ih, ow, oh):
    PAR.test_lanczos_paths_match_oracle(ctx, iw, ih, ow, oh)


# ---- full size: rows of 1920 and 1280 x 4 bytes have no padding at all, the end of the plane is the only place an overrun could go -----
@pytest.fixture(params=["guarded", "view", "skewed"])
def layout_full(request, ctx, monkeypatch):
    p = Placing(ctx, monkeypatch, request.param)
    yield p
    p.sweep()


def test_headline_tick_full_size(ctx, layout_full):
    """4 x 1080p NV12 -> 720p BGRA"""
    specs = [("img_nv12_bgra", 1920, 1080, dict(opacity=op)) for op in (1.0, 0.75, 0.5, 0.25)]
    MIX.run_tick_case(ctx, 1280, 720, True, specs, seed=0x5EED0000, expect=None)


@pytest.mark.parametrize("d", ["y420p", "nv12"])
def test_mixer_scene_full_size(ctx, switch, layout_full, d):
    switch("CHV_YUV_STREAM", "0")
    specs = [(f"img_{d}_{d}", 1920, 1080, dict()),
             (f"img_bgra_{d}", 640, 360, dict(rect=(64, 64, 640, 360), opacity=0.8)),
             (f"img_bgra_{d}", 640, 360, dict(rect=(1200, 640, 640, 360), opacity=0.6))]
    YWV.run_yuv_tick(ctx, d, 1920, 1080, True, specs, seed=0x5EED0000 + 64, expect=None)


# ---- the check can fail on the device ---------------------------------------------------------------------------------------------------
def test_positive_control_one_guard_byte(ctx, monkeypatch):
    placing = Placing(ctx, monkeypatch, "guarded")
    sample = placing.place("nv12", 50, 22, util.alloc_image("nv12", 50, 22, seed=8))
    pl = placing.rec.placement(sample)
    entry = placing.rec.entries[0]
    p = pl.planes[0]
    byte = p.offset + 7 * p.pitch + p.row + 2                          # pitch padding of row 7
    other = np.array([int(entry["want"][byte]) ^ 0x5A], dtype=np.uint8)
    cv.check(cv.load().chv_upload(ctx.handle, entry["buffer"]._h, byte, 1, other.ctypes.data, 1, 1, 1, 0))
    with pytest.raises(AssertionError) as err:
        placing.sweep()
    assert f"first at byte {byte}:" in str(err.value) and L.PADDING in str(err.value) and "behind row 7, 2 byte(s) past" in str(err.value), str(err.value)
    assert placing.sweep() == 0                                         # (the recorder is empty again)


def test_zz_routes_seen(ctx):
    """the kernel names the batches of this file were launched through, per layout (printed: run with -s).  Runs last in the file; when the
    whole file ran, every layout must have shown batches"""
    for name in L.LAYOUTS:
        print(f"\nlayout {name}: " + ", ".join(f"{k} x{n}" for k, n in sorted(ROUTES_SEEN.get(name, {}).items())))
    if len(ROUTES_SEEN) == len(L.LAYOUTS):
        for name in ("guarded", "view", "packed16"):
            assert any("stream" in k for k in ROUTES_SEEN[name]) and any("wave" in k for k in ROUTES_SEEN[name]) and any("tiled" in k for k in ROUTES_SEEN[name])
        assert not any(k.startswith(("tick_bgra_stream", "tick_yuv_stream")) or "tiled" in k for k in ROUTES_SEEN["skewed"]), ROUTES_SEEN["skewed"]
