"""chv_batch_rebind: an existing batch pointed at new pictures (include/chipvideo.h).

A host's upload ring and canvas ring rotate every tick (mix.video.swift:148-165), so the batch of a group tick never sees the same pictures
twice; between two ticks of a scene nothing but plane addresses changes.  Everything here goes through the C ABI and is held against the
oracle bit for bit, with both mechanisms (CHV_REBIND=scatter: the scatter kernel, kernels_rebind.hip.cpp; copy: the whole descriptor block
again): one batch per route chv_batch_create can choose, partial rebinds, views inside larger parents with guard bands, stream ordering
without host waits and across contexts, every refusal (after which the batch runs as before), VideoMixerGroup(reuseBatches=True) against the
default group, and one timing check against the path the library offered before (create + run + destroy per group tick)."""
import ctypes as C
import statistics
import time

import numpy as np
import pytest

import gpuutil as G
import layouts as L
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv

pytestmark = pytest.mark.gpu

K = sv.defaultComputeKernelFromString
VID4 = [("img_nv12_bgra", 480, 270, dict(opacity=o)) for o in (1.0, 0.75, 0.5, 0.25)]
LOGO = ("img_rgba_bgra_tx", 80, 44, dict(rect=(200, 20, 80, 44), rotation=0.3, opacity=0.9))

# name: (canvas format, w, h, [(kernel, src w, h, make_uniforms kwargs [+ csc])], switches, what chv_batch_describe must say, picture layout)
ROUTES = {
    "stream_opaque_bottom": ("bgra", 320, 180, VID4, {}, "tick_bgra_stream", None),
    "stream_bt601_full": ("bgra", 320, 180, [(k, w, h, dict(kw, csc=2)) for k, w, h, kw in VID4], {}, "tick_bgra_stream", None),
    "stream_plus_wave": ("bgra", 320, 180, VID4 + [LOGO], {}, "tick_bgra_stream + tick_bgra_wave", None),
    "tiled": ("bgra", 320, 180, [("img_nv12_bgra", 480, 270, dict())], {"CHV_BGRA_PATH": "tiled"}, "tick_nv12_bgra_tiled", None),
    "wave_mixed": ("bgra", 320, 180, [("img_nv12_bgra", 480, 270, dict()), ("img_y420p_bgra", 160, 90, dict(rect=(20, 16, 160, 90), opacity=0.8)),
                                      ("img_bgra_bgra_tx", 96, 54, dict(rect=(180, 100, 120, 60), opacity=0.6, border=(3, 3, 3, 3), fill=(0.1, 0.9, 0.2, 0.7))), LOGO],
                   {"CHV_BGRA_PATH": "wave"}, "tick_bgra_wave", None),
    "wave_rgb_only": ("bgra", 320, 180, [("img_bgra_bgra_tx", 320, 180, dict()), ("img_rgba_bgra_tx", 96, 54, dict(rect=(40, 30, 96, 54), opacity=0.7))],
                      {"CHV_BGRA_PATH": "wave"}, "tick_bgra_wave", None),
    "yuv_wave_nv12": ("nv12", 320, 180, [("img_nv12_nv12", 480, 270, dict()), ("img_bgra_nv12", 96, 54, dict(rect=(30, 20, 120, 70), opacity=0.7))],
                      {"CHV_YUV_STREAM": "0"}, "tick_yuv_wave<nv12>", None),
    "yuv_wave_y420p": ("y420p", 320, 180, [("img_y420p_y420p", 480, 270, dict()), ("img_rgba_y420p", 96, 54, dict(rect=(30, 20, 120, 70), opacity=0.7))],
                       {"CHV_YUV_STREAM": "0"}, "tick_yuv_wave<y420p>", None),
    "encoder_frame": ("nv12", 320, 180, [("img_bgra_nv12_int", 320, 180, dict())], {"CHV_YUV_STREAM": "force"}, "tick_yuv_stream<nv12>", None),
    "general_odd_unaligned": ("bgra", 131, 77, [("img_nv12_bgra", 94, 50, dict(rect=(5, 3, 120, 70))), ("img_rgba_bgra_tx", 33, 21, dict(rect=(60, 30, 50, 40), rotation=0.2, opacity=0.8))],
                              {"CHV_FORCE_GENERAL": "1"}, "tick_general_bgra", "skewed"),
    "general_yuv_odd": ("y420p", 130, 78, [("img_y420p_y420p", 94, 50, dict(rect=(5, 3, 120, 70))), ("img_bgra_y420p", 33, 21, dict(rect=(60, 30, 50, 40), opacity=0.8))],
                        {"CHV_FORCE_GENERAL": "1"}, "tick_general_yuv<y420p>", "skewed"),
    "eighteen_layers": ("bgra", 192, 96, [("img_nv12_bgra", 192, 96, dict())] +
                        [("img_bgra_bgra_tx", 40, 24, dict(rect=(8 * i, 4 * i, 48, 28), opacity=0.5 + 0.02 * i)) for i in range(17)], {}, None, None),
}


class Pictures:
    """one set of pictures for a scene: sources and canvases on the device, their host copies, the oracle's canvases"""

    def __init__(self, ctx, scene, seed, n_ticks=3, layout=None, recorder=None):
        dst, cw, ch, specs = scene[:4]
        layout = layout or scene[6]
        self.dst, self.cw, self.ch, self.specs = dst, cw, ch, specs
        self.ticks, self.exps, self.gds, self.srcs, self.canvas0 = [], [], [], [], []
        self.n = 0

        def put(fmt, w, h, planes):
            self.n += 1
            if layout is None:
                return G.to_gpu(ctx, fmt, w, h, planes)
            # (skewed pitches and view positions follow the seed: sets that replace one another keep seed % 24, so that only addresses differ)
            return L.place(ctx, fmt, w, h, planes, layout, seed=24 * (seed * 64 + self.n) + 5, recorder=recorder)

        for t in range(n_ticks):
            canvas0 = util.alloc_image(dst, cw, ch, seed=seed * 1000 + t)
            layers, srcs = [], []
            for i, (k, sw, sh, kw) in enumerate(specs):
                kw = dict(kw)
                csc = kw.pop("csc", 0)
                s = k.split("_")[1]
                src = util.alloc_image(s, sw, sh, seed=seed * 1000 + 100 + 31 * t + i)
                srcs.append(src)
                layers.append((K(k), put(s, sw, sh, src), util.make_uniforms((cw, ch), in_size=(sw, sh), **kw), csc))
            gd = put(dst, cw, ch, canvas0)
            self.ticks.append((gd, True, layers)); self.gds.append(gd); self.srcs.append(srcs); self.canvas0.append(canvas0)
            self.exps.append(self.oracle(srcs))

    def oracle(self, srcs):
        """the canvas of one tick of this scene whose layers show `srcs`"""
        exp = util.alloc_image(self.dst, self.cw, self.ch)
        assert O.run_kernel(f"img_clear_{self.dst}", exp) == 0
        for (k, sw, sh, kw), src in zip(self.specs, srcs):
            kw = dict(kw)
            csc = kw.pop("csc", 0)
            assert O.run_kernel(k, exp, src, util.make_uniforms((self.cw, self.ch), in_size=(sw, sh), **kw), csc=csc, threads=4) == 0
        return exp

    def check(self, ctx, what, exps=None, from_gpu=None):
        for t, (gd, exp) in enumerate(zip(self.gds, exps or self.exps)):
            G.assert_same((from_gpu or G.from_gpu)(ctx, gd, self.dst, self.cw, self.ch), exp, f"{what}, tick {t}")

    def scribble(self, ctx, seed):
        """noise into every canvas (a cleared tick does not read it): a run that did not reach a canvas shows"""
        lib = cv.load()
        noise = []
        for t, gd in enumerate(self.gds):
            img = gd.imageBuffer()
            planes = util.alloc_image(self.dst, self.cw, self.ch, seed=seed * 77 + t)
            for i, a in enumerate(planes):
                a2 = np.ascontiguousarray(a).reshape(a.shape[0], -1)
                cv.check(lib.chv_upload(ctx.handle, img.computeTextures[i]._h, img.gpuOffsets[i], img.gpuPitches[i], a2.ctypes.data, a2.shape[1], a2.shape[1], a2.shape[0], 0))
            noise.append(planes)
        return noise

    def all_items(self, targets=True, layers=True):
        out = []
        for t, (gd, _, ls) in enumerate(self.ticks):
            if targets:
                out.append((t, -1, gd))
            if layers:
                out += [(t, l, s) for l, (_, s, _, _) in enumerate(ls)]
        return out


def rebind_array(items):
    arr = (cv.Rebind * max(1, len(items)))()
    for i, (t, l, sample) in enumerate(items):
        arr[i].tick, arr[i].layer, arr[i].image = t, l, sv._image_desc(sample)
    return arr


def rebind(ctx, h, items):
    arr = rebind_array(items)
    return cv.load().chv_batch_rebind(ctx.handle, h, arr, len(items))


def enqueue(ctx, h, wait=0):
    lib = cv.load()
    cv.check(lib.chv_pass_begin(ctx.handle)); cv.check(lib.chv_batch_run(ctx.handle, h)); cv.check(lib.chv_pass_end(ctx.handle, wait))


def describe(h):
    name, n = C.create_string_buffer(128), C.c_int(0)
    cv.check(cv.load().chv_batch_describe(h, name, 128, C.byref(n)))
    return name.value.decode(), n.value


@pytest.fixture(params=["scatter", "copy"])
def mechanism(request, switch):
    switch("CHV_REBIND", request.param)
    return request.param


def test_the_library_carries_the_scatter_kernel(built):
    assert "batch_rebind:scatter=1" in cv.build_flags()


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_follows_its_pictures(ctx, switch, mechanism, route):
    """A: build, run.  B: rebind everything, run — the oracle's canvases, the bytes of a fresh batch over B, A's canvases untouched.  Back to A."""
    scene = ROUTES[route]
    for name, value in scene[4].items():
        switch(name, value)
    a, b, b2 = Pictures(ctx, scene, 1), Pictures(ctx, scene, 2), Pictures(ctx, scene, 2)
    h, name, keep = G.make_batch(ctx, a.ticks)
    try:
        if scene[5] is not None:
            assert name == scene[5], name
        n_launches = describe(h)[1]
        assert n_launches == (2 if " + " in name else 1)
        G.run_batch(ctx, h)
        a.check(ctx, f"{route}: set A via {name}")
        assert rebind(ctx, h, b.all_items()) == 0, cv.load().chv_last_error_detail()
        G.run_batch(ctx, h)
        b.check(ctx, f"{route}: set B after the rebind ({mechanism})")
        a.check(ctx, f"{route}: set A after the batch has moved on to B")
        h2, name2, keep2 = G.make_batch(ctx, b2.ticks)
        G.run_batch(ctx, h2)
        G.destroy_batch(h2)
        assert name2 == name
        for t in range(len(b.gds)):
            G.assert_same(G.from_gpu(ctx, b.gds[t], b.dst, b.cw, b.ch), G.from_gpu(ctx, b2.gds[t], b.dst, b.cw, b.ch), f"{route}: rebound batch against a fresh one, tick {t}")
        assert describe(h) == (name, n_launches)
        # back to A: its canvases hold noise now, the ones of B the result they had
        a.scribble(ctx, 3)
        assert rebind(ctx, h, a.all_items()) == 0
        G.run_batch(ctx, h)
        G.run_batch(ctx, h)              # (strip routes build their geometry tables at a batch's second launch with a configuration: the layers travel again)
        a.check(ctx, f"{route}: back on set A")
        b.check(ctx, f"{route}: set B after the batch has gone back to A")
    finally:
        G.destroy_batch(h)


def test_the_last_layer_of_a_deep_tick(ctx, mechanism):
    """positions count within the tick as given to chv_batch_create, beyond 16 layers too"""
    scene = ROUTES["eighteen_layers"]
    a, b = Pictures(ctx, scene, 4), Pictures(ctx, scene, 5)
    h, name, keep = G.make_batch(ctx, a.ticks)
    try:
        assert rebind(ctx, h, [(1, 17, b.ticks[1][2][17][1])]) == 0
        G.run_batch(ctx, h)
        exps = list(a.exps)
        exps[1] = a.oracle(a.srcs[1][:17] + [b.srcs[1][17]])
        a.check(ctx, f"layer 17 of tick 1 rebound ({name})", exps)
        assert rebind(ctx, h, [(1, 18, b.ticks[1][2][17][1])]) == 1
    finally:
        G.destroy_batch(h)


@pytest.mark.parametrize("route", ["stream_opaque_bottom", "stream_plus_wave", "yuv_wave_y420p", "general_odd_unaligned"])
def test_partial_rebinds(ctx, switch, mechanism, route):
    scene = ROUTES[route]
    for name, value in scene[4].items():
        switch(name, value)
    a, b = Pictures(ctx, scene, 6), Pictures(ctx, scene, 7)
    h, name, keep = G.make_batch(ctx, a.ticks)
    try:
        # targets only: A's pictures land on B's canvases, A's canvases keep their noise
        noise = a.scribble(ctx, 8)
        assert rebind(ctx, h, b.all_items(layers=False)) == 0
        G.run_batch(ctx, h)
        b.check(ctx, f"{route}: targets only", a.exps)
        a.check(ctx, f"{route}: the canvases rebound away", noise)
        # one layer of one tick (the last tick's first layer): everything else stays
        assert rebind(ctx, h, [(2, 0, b.ticks[2][2][0][1])]) == 0
        G.run_batch(ctx, h)
        exps = list(a.exps)
        exps[2] = a.oracle([b.srcs[2][0]] + a.srcs[2][1:])
        b.check(ctx, f"{route}: one layer of one tick", exps)
    finally:
        G.destroy_batch(h)


@pytest.mark.parametrize("route", ["stream_opaque_bottom", "wave_mixed", "yuv_wave_nv12"])
def test_views_inside_larger_parents(ctx, switch, mechanism, route):
    """planes as views at non-zero offsets of larger parents of equal pitch; every allocation is read back whole afterwards: payload of the
    targets bound at the time of a run and nothing else may have changed"""
    scene = ROUTES[route]
    for name, value in scene[4].items():
        switch(name, value)
    rec = L.Recorder()
    a, b = Pictures(ctx, scene, 9, layout="view", recorder=rec), Pictures(ctx, scene, 10, layout="view", recorder=rec)
    from_gpu = lambda c, s, fmt, w, h: L.from_gpu(rec, G.from_gpu, c, s, fmt, w, h)      # noqa: E731
    h, name, keep = G.make_batch(ctx, a.ticks)
    try:
        assert name == scene[5], name
        G.run_batch(ctx, h)
        assert rebind(ctx, h, b.all_items()) == 0, cv.load().chv_last_error_detail()
        G.run_batch(ctx, h)
        a.check(ctx, f"{route}: views, set A", from_gpu=from_gpu)
        b.check(ctx, f"{route}: views, set B", from_gpu=from_gpu)
    finally:
        G.destroy_batch(h)
    assert rec.sweep(ctx) > 0


def test_rebind_run_rebind_run_then_one_wait(ctx, mechanism):
    scene = ROUTES["stream_plus_wave"]
    a, b, c = Pictures(ctx, scene, 11), Pictures(ctx, scene, 12), Pictures(ctx, scene, 13)
    h, name, keep = G.make_batch(ctx, a.ticks)
    try:
        for rep in range(3):
            for p in (a, b, c):
                p.scribble(ctx, 14 + rep)
            enqueue(ctx, h)
            assert rebind(ctx, h, b.all_items()) == 0
            enqueue(ctx, h)
            assert rebind(ctx, h, c.all_items()) == 0
            enqueue(ctx, h)
            assert rebind(ctx, h, a.all_items()) == 0
            cv.check(cv.load().chv_pass_end(ctx.handle, 1))
            for p, what in ((a, "A"), (b, "B"), (c, "C")):
                p.check(ctx, f"run, rebind(B), run, rebind(C), run, rebind(A), one wait: set {what}, round {rep}")
    finally:
        G.destroy_batch(h)


def test_a_long_list_twice_without_a_wait(ctx, switch):
    """more than the kernel arguments hold (220 pairs): the list is staged in pinned memory of the batch, two areas in turn"""
    switch("CHV_REBIND", "scatter")
    scene = ("bgra", 64, 32, [("img_nv12_bgra", 96, 48, dict(opacity=o)) for o in (1.0, 0.5)], {}, "tick_bgra_stream", None)
    sets = [Pictures(ctx, scene, 20 + i, n_ticks=60) for i in range(4)]          # 60 x (1 + 2 x 2) planes = 300 pairs
    h, name, keep = G.make_batch(ctx, sets[0].ticks)
    try:
        enqueue(ctx, h)
        for p in sets[1:]:
            assert rebind(ctx, h, p.all_items()) == 0
            enqueue(ctx, h)
        cv.check(cv.load().chv_pass_end(ctx.handle, 1))
        for i, p in enumerate(sets):
            p.check(ctx, f"set {i} of four, 300 pairs per rebind")
    finally:
        G.destroy_batch(h)


def test_a_frame_uploaded_asynchronously_through_another_context(ctx, mechanism):
    """upload(async=1) on a second context, rebind + run on the first with no host wait between: the run waits for the copies of the buffers
    bound NOW"""
    lib = cv.load()
    scene = ROUTES["stream_opaque_bottom"]
    a, b, fresh = Pictures(ctx, scene, 30), Pictures(ctx, scene, 31), Pictures(ctx, scene, 32)
    up = sv.createComputeContext(sharing=ctx)
    h, name, keep = G.make_batch(ctx, a.ticks)
    try:
        G.run_batch(ctx, h)
        # B's buffers receive `fresh`'s pixels on the uploader's stream ...
        for t, (_, _, layers) in enumerate(b.ticks):
            for l, (_, sample, _, _) in enumerate(layers):
                img = sample.imageBuffer()
                for i, plane in enumerate(fresh.srcs[t][l]):
                    p2 = np.ascontiguousarray(plane).reshape(plane.shape[0], -1)
                    cv.check(lib.chv_upload(up.handle, img.computeTextures[i]._h, img.gpuOffsets[i], img.gpuPitches[i], p2.ctypes.data, p2.shape[1], p2.shape[1], p2.shape[0], 1))
        # ... and the batch moves on to them at once
        assert rebind(ctx, h, b.all_items()) == 0
        enqueue(ctx, h, wait=1)
        b.check(ctx, "rebind + run behind an asynchronous upload", fresh.exps)
    finally:
        G.destroy_batch(h)
        sv.destroyComputeContext(up)


def test_created_on_one_context_rebound_on_a_second_run_on_a_third(ctx, mechanism):
    scene = ROUTES["wave_mixed"]
    c2, c3 = sv.createComputeContext(sharing=ctx), sv.createComputeContext(sharing=ctx)
    a, b = Pictures(ctx, scene, 33), Pictures(ctx, scene, 34)
    h, name, keep = G.make_batch(ctx, a.ticks)
    try:
        for rep in range(3):
            a.scribble(ctx, 35 + rep); b.scribble(ctx, 36 + rep)
            enqueue(ctx, h)                                      # (A, on the creator's stream: not waited for)
            assert rebind(c2, h, b.all_items()) == 0
            enqueue(c3, h, wait=1)
            assert rebind(c3, h, a.all_items()) == 0
            cv.check(cv.load().chv_pass_end(ctx.handle, 1))
            a.check(ctx, f"set A, run on the creator's stream before the rebind (round {rep})")
            b.check(ctx, f"set B, rebound on a second context and run on a third (round {rep})")
    finally:
        G.destroy_batch(h)
        sv.destroyComputeContext(c2); sv.destroyComputeContext(c3)


# ---- refusals: the code, and a run that reproduces what the batch did before the call ------------------------------------------------------
WIDE = ("bgra", 320, 180, [("img_nv12_bgra", 512, 288, dict(opacity=o)) for o in (1.0, 0.5)], {}, "tick_bgra_stream", None)      # rows of 512 bytes: every layout's pitch


def _desc(sample, **plane0):
    d = sv._image_desc(sample)
    for k, v in plane0.items():
        setattr(d.planes[0], k, v)
    return d


def test_refusals_leave_the_batch_as_it_was(ctx, mechanism):
    lib = cv.load()
    a, b = Pictures(ctx, WIDE, 40), Pictures(ctx, WIDE, 41)
    h, name, keep = G.make_batch(ctx, a.ticks)
    rec = L.Recorder()
    nv = lambda w, hh, seed: util.alloc_image("nv12", w, hh, seed=seed)      # noqa: E731
    good = b.ticks[0][2][0][1]
    bad = {
        "another size": (G.to_gpu(ctx, "nv12", 480, 270, nv(480, 270, 1)), (1,)),
        "another pitch": (L.place(ctx, "nv12", 512, 288, nv(512, 288, 2), "view", seed=3, recorder=rec), (1,)),
        "another format": (G.to_gpu(ctx, "y420p", 512, 288, util.alloc_image("y420p", 512, 288, seed=4)), (1,)),
        "an address of another alignment": (L.place(ctx, "nv12", 512, 288, nv(512, 288, 5), "at4p0", seed=6, recorder=rec), (1,)),
    }
    try:
        assert name == WIDE[5]
        G.run_batch(ctx, h)
        a.check(ctx, "set A")

        def unchanged(what):
            a.scribble(ctx, 42)
            G.run_batch(ctx, h)
            a.check(ctx, f"after a refused rebind ({what})")

        for what, (sample, codes) in bad.items():
            rc = rebind(ctx, h, [(1, 0, sample)])
            assert rc in codes, (what, rc, lib.chv_last_error_detail())
            assert b"rebuild the batch" in lib.chv_last_error_detail(), (what, lib.chv_last_error_detail())
            unchanged(what)
        # a component count the slot's kernel does not read: the code chv_batch_create gives for such a plane
        arr = rebind_array([(1, 0, good)])
        arr[0].image = _desc(good, components=2)
        assert lib.chv_batch_rebind(ctx.handle, h, arr, 1) == 5
        arr = rebind_array([(1, -1, b.gds[1])])
        arr[0].image = _desc(b.gds[1], components=1)
        assert lib.chv_batch_rebind(ctx.handle, h, arr, 1) == 4
        # an extent beyond the buffer
        arr = rebind_array([(1, 0, good)])
        arr[0].image = _desc(good, offset=1 << 20)
        assert lib.chv_batch_rebind(ctx.handle, h, arr, 1) == 5
        unchanged("bad planes")
        for t, l in ((-1, 0), (3, 0), (0, 2), (0, -2), (1 << 20, -1)):
            assert rebind(ctx, h, [(t, l, good)]) == 1, (t, l)
        assert rebind(ctx, h, [(0, 0, good), (1, 1, good), (0, 0, b.ticks[0][2][1][1])]) == 1 and b"twice" in lib.chv_last_error_detail()
        assert rebind(ctx, h, [(2, -1, b.gds[2]), (2, -1, b.gds[1])]) == 1
        assert lib.chv_batch_rebind(ctx.handle, h, None, 1) == 1
        assert lib.chv_batch_rebind(ctx.handle, None, rebind_array([(0, 0, good)]), 1) == 1
        assert lib.chv_batch_rebind(None, h, rebind_array([(0, 0, good)]), 1) == 3
        unchanged("indices, duplicates, null pointers")
        # [valid, invalid]: the valid one has not been applied
        noise = b.scribble(ctx, 43)
        assert rebind(ctx, h, [(0, -1, b.gds[0]), (0, 0, good), (1, 0, bad["another size"][0])]) == 1
        unchanged("a valid item in front of an invalid one")
        b.check(ctx, "the canvas a refused list named", noise)
        # ... and the batch still takes a good list
        assert rebind(ctx, h, b.all_items()) == 0
        G.run_batch(ctx, h)
        b.check(ctx, "set B after the refusals")
    finally:
        G.destroy_batch(h)
    rec.sweep(ctx)


def test_the_general_route_takes_any_address(ctx, switch, mechanism):
    """no alignment condition on the general kernels: a picture 4 bytes off takes the place of an aligned one of the same pitch"""
    switch("CHV_FORCE_GENERAL", "1")
    a, b = Pictures(ctx, WIDE, 44, n_ticks=1), Pictures(ctx, WIDE, 45, n_ticks=1)
    rec = L.Recorder()
    src = util.alloc_image("nv12", 512, 288, seed=46)
    off = L.place(ctx, "nv12", 512, 288, src, "at4p0", seed=7, recorder=rec)
    h, name, keep = G.make_batch(ctx, a.ticks)
    try:
        assert name == "tick_general_bgra"
        assert rebind(ctx, h, [(0, -1, b.gds[0]), (0, 1, off)]) == 0, cv.load().chv_last_error_detail()
        G.run_batch(ctx, h)
        b.check(ctx, "a source at 4 mod 16 on the general route", [a.oracle([a.srcs[0][0], src])])
    finally:
        G.destroy_batch(h)
    rec.sweep(ctx)


# ---- the hosts ---------------------------------------------------------------------------------------------------------------------------
def _mixer_layer(ctx, fmt, w, h, seed, canvas, rect, z, opacity=1.0, asset="cam"):
    """(revision = the asset: a new frame of a source takes the place of its last one in the mixer, mix.video.swift:57-75)"""
    M = util.ortho(*canvas) @ util._mat_translate(rect[0], rect[1]) @ util._mat_scale(rect[2], rect[3])
    p = sv.pictureFromArrays(G.FMT[fmt], (w, h), util.alloc_image(fmt, w, h, seed=seed), matrix=M, opacity=opacity, zIndex=z, assetId=asset, revision=asset)
    return sv.uploadComputePicture(ctx, p)


def test_mixer_group_that_keeps_its_batches(ctx):
    """VideoMixerGroup(reuseBatches=True) over rotating rings for more than ten ticks equals the default group tick by tick; a scene change in
    the middle (one layer resized) builds afresh and still matches"""
    specs = [("nv12", (96, 54)), ("y420p", (64, 36)), ("bgra", (80, 44)), ("bgra", (80, 44))]
    kept, plain = [], []
    for k, (fmt, canvas) in enumerate(specs):
        for dest in (kept, plain):
            dest.append(sv.VideoMixer("ws", 1 / 30, canvas, outputFormat=G.FMT[fmt], computeContext=ctx, assetId=f"mixer{k}"))
    g_kept, g_plain = sv.VideoMixerGroup(kept, reuseBatches=True), sv.VideoMixerGroup(plain)
    assert g_plain.reuseBatches is False
    ring = {}
    try:
        for tick in range(14):
            for k, (fmt, canvas) in enumerate(specs):
                src_fmt = "nv12" if fmt != "y420p" else "y420p"
                logo = (8, 6, 30, 20) if tick < 8 else (8, 6, 36, 24)          # the scene changes at tick 8
                for dest in (kept, plain):
                    # (an upload ring of three: the pictures of tick t come back at tick t + 3 with new pixels only in a real host; here new uploads)
                    ring[(tick % 3, k, id(dest))] = [_mixer_layer(ctx, src_fmt, 48, 30, 100 * tick + k, canvas, (0, 0) + canvas, 0),
                                                     _mixer_layer(ctx, "bgra", 20, 16, 100 * tick + 50 + k, canvas, logo, 1, opacity=0.7, asset="logo")]
                    for pic in ring[(tick % 3, k, id(dest))]:
                        dest[k].push(pic)
            outs, refs = g_kept.mix(at=0.0), g_plain.mix(at=0.0)
            assert outs is not None and refs is not None, ([m.result for m in kept], [m.result for m in plain])
            for k, ((fmt, canvas), out, ref) in enumerate(zip(specs, outs, refs)):
                G.assert_same(G.from_gpu(ctx, out, fmt, *canvas), G.from_gpu(ctx, ref, fmt, *canvas), f"tick {tick}, mixer {k} ({fmt})")
        # three canvas formats: built at tick 0 and at tick 8, rebound at every other tick
        assert (g_kept.rebuilds, g_kept.rebinds) == (6, 36), (g_kept.rebuilds, g_kept.rebinds)
    finally:
        g_kept.destroy()


def test_rebind_and_run_is_no_slower_than_building_the_batch(ctx):
    """256 headline ticks (four 1080p NV12 pictures onto a 720p BGRA canvas each) over two picture sets: 20 alternations of (rebind everything +
    run + wait) and (create + run + wait + destroy), the group tick the library offered before.  A set has 256 canvases of its own; its ticks
    share four source pictures (fewer distinct buffers than a host's ring: the descriptors, the list of 2 304 planes and the launch are the
    headline's).  Measured on one MI355X: 1067.9 against 1102.1 us."""
    lib = cv.load()
    sets = []
    for s in range(2):
        srcs = [G.to_gpu(ctx, "nv12", 1920, 1080, util.alloc_image("nv12", 1920, 1080, seed=50 + 4 * s + i)) for i in range(4)]
        # 256 canvases: the launch writes every one of them
        gds = [G.to_gpu(ctx, "bgra", 1280, 720, util.alloc_image("bgra", 1280, 720)) for _ in range(256)]
        us = [util.full_canvas_uniforms((1280, 720), (1920, 1080), opacity=o) for o in (1.0, 0.75, 0.5, 0.25)]
        sets.append([(gd, True, [(K("img_nv12_bgra"), srcs[i], us[i], 0) for i in range(4)]) for gd in gds])
    arrays = []
    for ticks in sets:
        arr = (cv.Tick * 256)()
        keep = []
        for i, (gd, clear, layers) in enumerate(ticks):
            la = sv._layer_array(layers)
            keep.append(la)
            arr[i].target, arr[i].clear_first, arr[i].n_layers, arr[i].layers = sv._image_desc(gd), 1, 4, la
        arrays.append((arr, keep))
    items = [rebind_array([(t, -1, gd) for t, (gd, _, _) in enumerate(ticks)] + [(t, l, s) for t, (_, _, ls) in enumerate(ticks) for l, (_, s, _, _) in enumerate(ls)])
             for ticks in sets]
    h = C.c_void_p()
    cv.check(lib.chv_batch_create(ctx.handle, arrays[0][0], 256, C.byref(h)))
    assert describe(h)[0] == "tick_bgra_stream"

    def rebound(k):
        t0 = time.perf_counter()
        cv.check(lib.chv_batch_rebind(ctx.handle, h, items[k], 256 * 5))      # 256 canvases + 1 024 pictures = 2 304 planes
        cv.check(lib.chv_batch_run(ctx.handle, h))
        cv.check(lib.chv_pass_end(ctx.handle, 1))
        return time.perf_counter() - t0

    def fresh(k):
        t0 = time.perf_counter()
        hb = C.c_void_p()
        cv.check(lib.chv_batch_create(ctx.handle, arrays[k][0], 256, C.byref(hb)))
        cv.check(lib.chv_batch_run(ctx.handle, hb))
        cv.check(lib.chv_pass_end(ctx.handle, 1))
        cv.check(lib.chv_batch_destroy(hb))
        return time.perf_counter() - t0

    try:
        for k in range(4):
            rebound(k & 1); fresh(k & 1)            # warm: pool blocks, pinned lists
        tr, tf = [], []
        for k in range(20):
            tr.append(rebound(k & 1)); tf.append(fresh(k & 1))
        mr, mf = statistics.median(tr) * 1e6, statistics.median(tf) * 1e6
        print(f"\n256 headline ticks: rebind + run + wait {mr:.1f} us, create + run + wait + destroy {mf:.1f} us (medians of 20, alternating)")
        assert mr <= mf, (mr, mf)
    finally:
        cv.check(lib.chv_batch_destroy(h))
