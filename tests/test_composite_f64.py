"""The compositing kernels' restatement against an independent float64 statement (tests/composite_f64.py; DESIGN.md sections 4.1 - 4.3, 4.5
and the reference's own kernels on 4:2:0 canvases, the float RGB -> YUV ones included).

Every bit-exact GPU test of the tick kernels builds its expectation from oracle/ref_kernels.c, which was written from the same reading of the
formulas as the kernels.  Here the oracle is held to the statement's intervals (a) on named cases, each at the smallest size that still has
its feature, (b) on seeded cases in the style of the fuzzers, singly and in stacks of 2 - 4 mixed layers on cleared and seeded canvases;
(c) wrong statements of the arithmetic are shown to FAIL far outside the intervals; (d) the caps on what the intervals may hide are asserted
from the statement alone.  tests/test_gpu_composite_f64.py compares the kernels themselves, route by route, on the same cases."""
import functools

import numpy as np
import pytest

import composite_f64 as F
import util
from lanczos_f64 import assert_within
from oracle import oracle as O

BGRA_KERNELS = ["img_nv12_bgra", "img_y420p_bgra", "img_bgra_bgra_tx", "img_rgba_bgra_tx"]
YUV_KERNELS = {"nv12": ["img_nv12_nv12", "img_y420p_nv12", "img_bgra_nv12_int", "img_rgba_nv12_int"],
               "y420p": ["img_y420p_y420p", "img_bgra_y420p_int", "img_rgba_y420p_int"]}
# the float RGB -> YUV kernels draw from lists of their own (beside a video layer to lie over), so that the lists above draw what they always drew
PREMUL_KERNELS = {"nv12": ["img_bgra_nv12", "img_rgba_nv12", "img_nv12_nv12"], "y420p": ["img_bgra_y420p", "img_rgba_y420p", "img_y420p_y420p"]}


def L(kernel, iw, ih, seed, csc=0, **kw):
    """one layer: kernel, source size, source seed, colourspace, util.make_uniforms' arguments"""
    return (kernel, iw, ih, seed, csc, tuple(sorted(kw.items())))


def case(fmt, W, H, layers, canvas_seed=None):
    """a tick: canvas_seed None clears the canvas first (section 4.3), otherwise the canvas starts from seeded bytes"""
    return (fmt, W, H, canvas_seed, tuple(layers))


# ---- a. named cases ----------------------------------------------------------------------------------------------------------------------------
NAMED = {
    # general fractional scale, up and down
    "up-nv12": case("bgra", 37, 23, [L("img_nv12_bgra", 22, 14, 1)], 3),
    "down-y420p": case("bgra", 31, 19, [L("img_y420p_bgra", 86, 50, 2, csc=1)], 4),
    "up-bgra": case("bgra", 29, 17, [L("img_bgra_bgra_tx", 13, 9, 3, opacity=0.7)], 5),
    "down-rgba": case("bgra", 23, 21, [L("img_rgba_bgra_tx", 61, 47, 4)], 6),
    "up-int": case("y420p", 30, 18, [L("img_bgra_y420p_int", 13, 9, 90, csc=2)], 91),
    "down-int": case("nv12", 22, 14, [L("img_rgba_nv12_int", 61, 47, 92, csc=1, opacity=0.65)], 93),
    # a layer across each canvas edge
    "left-top": case("bgra", 40, 26, [L("img_nv12_bgra", 30, 20, 5, rect=(-9.3, -5.7, 31.1, 20.9))], 7),
    "right-bottom": case("bgra", 40, 26, [L("img_rgba_bgra_tx", 30, 20, 6, rect=(20.6, 12.2, 33.3, 25.1))], 8),
    "left-top-420": case("nv12", 40, 26, [L("img_nv12_nv12", 30, 20, 7, rect=(-9.3, -5.7, 31.1, 20.9))], 9),
    "right-bottom-420": case("y420p", 40, 26, [L("img_y420p_y420p", 30, 20, 8, rect=(20.6, 12.2, 33.3, 25.1))], 10),
    # rotation
    "rotated-y420p": case("bgra", 48, 30, [L("img_y420p_bgra", 40, 24, 9, csc=2, rect=(12.0, 7.0, 26.0, 15.0), rotation=0.6)], 11),
    "rotated-bgra": case("bgra", 48, 30, [L("img_bgra_bgra_tx", 40, 24, 10, rect=(10.0, 6.0, 27.0, 16.0), rotation=-1.9, opacity=0.8)], 12),
    "rotated-int": case("nv12", 48, 30, [L("img_bgra_nv12_int", 40, 24, 11, csc=1, rect=(12.0, 7.0, 26.0, 15.0), rotation=2.4)], 13),
    # border plus fill with fill.a < 1
    "border-fill": case("bgra", 44, 28, [L("img_nv12_bgra", 24, 16, 12, rect=(9.3, 6.4, 22.1, 13.3), border=(3.2, 2.3, 4.1, 5.4),
                                           fill=(0.9, 0.3, 0.55, 0.6), opacity=0.75)], 14),
    "border-fill-rgba": case("bgra", 44, 28, [L("img_rgba_bgra_tx", 24, 16, 13, rect=(9.3, 6.4, 22.1, 13.3), border=(3.2, 2.3, 4.1, 5.4),
                                                fill=(0.2, 0.8, 0.4, 0.35))], 15),
    "border-fill-420": case("nv12", 44, 28, [L("img_y420p_nv12", 24, 16, 14, rect=(9.3, 6.4, 22.1, 13.3), border=(3.2, 2.3, 4.1, 5.4),
                                               fill=(0.9, 0.3, 0.55, 0.6), opacity=0.75)], 16),
    "border-fill-int": case("y420p", 44, 28, [L("img_rgba_y420p_int", 24, 16, 15, csc=3, rect=(9.3, 6.4, 22.1, 13.3), border=(3.2, 2.3, 4.1, 5.4),
                                                fill=(0.2, 0.8, 0.4, 0.35), opacity=0.9)], 17),
    # texture crop, horizontal flip
    "crop": case("bgra", 36, 22, [L("img_y420p_bgra", 50, 30, 16, csc=3, tex=(0.21, 0.13, 0.55, 0.62))], 18),
    "crop-outside": case("bgra", 36, 22, [L("img_bgra_bgra_tx", 50, 30, 17, tex=(-0.15, 0.3, 1.2, 0.9), fill=(0.13, 0.27, 0.91, 1.0))], 19),
    "flip": case("bgra", 36, 22, [L("img_nv12_bgra", 50, 30, 18, tex=(1.0, 0.0, -1.0, 1.0))], 20),
    "flip-420": case("nv12", 36, 22, [L("img_nv12_nv12", 50, 30, 19, tex=(1.0, 0.0, -1.0, 1.0), opacity=0.5)], 21),
    "flip-int": case("nv12", 36, 22, [L("img_rgba_nv12_int", 50, 30, 20, tex=(0.9, 0.1, -0.8, 0.8))], 22),
    # opacity 0, 1 and fractional
    "opacity-0": case("bgra", 19, 13, [L("img_rgba_bgra_tx", 14, 11, 21, opacity=0.0, fill=(1.0, 1.0, 1.0, 1.0))], 23),
    "opacity-1": case("bgra", 19, 13, [L("img_nv12_bgra", 14, 11, 22, opacity=1.0)], 24),
    "opacity-frac": case("bgra", 19, 13, [L("img_y420p_bgra", 14, 11, 23, opacity=0.3137)], 25),
    "opacity-frac-420": case("y420p", 22, 14, [L("img_y420p_y420p", 14, 11, 24, opacity=0.3137)], 26),
    # per-pixel alpha through several re-quantised layers
    "alpha-stack": case("bgra", 26, 18, [L("img_bgra_bgra_tx", 19, 13, 25), L("img_rgba_bgra_tx", 33, 21, 26, opacity=0.85),
                                         L("img_bgra_bgra_tx", 11, 7, 27, rect=(3.3, 2.4, 17.2, 12.1))], 27),
    "alpha-stack-int": case("y420p", 26, 18, [L("img_bgra_y420p_int", 19, 13, 28), L("img_rgba_y420p_int", 33, 21, 29, csc=2, opacity=0.85)], 28),
    # all four colourspaces
    **{f"csc{c}": case("bgra", 23, 13, [L("img_nv12_bgra", 32, 18, 30 + c, csc=c)], 29 + c) for c in range(4)},
    **{f"csc{c}-int": case("nv12", 26, 14, [L("img_bgra_nv12_int", 31, 17, 34 + c, csc=c)], 33 + c) for c in range(4)},
    # odd 4:2:0 canvases and sources
    "odd-nv12": case("nv12", 27, 15, [L("img_nv12_nv12", 21, 13, 40, opacity=0.6)], 41),
    "odd-y420p": case("y420p", 15, 27, [L("img_y420p_y420p", 13, 21, 42)], 43),
    "odd-int": case("nv12", 27, 15, [L("img_rgba_nv12_int", 21, 13, 44, rect=(-2.3, 1.2, 30.1, 15.3))], 45),
    "odd-source-bgra": case("bgra", 27, 15, [L("img_y420p_bgra", 21, 13, 46)], 47),
    "smallest": case("bgra", 7, 5, [L("img_nv12_bgra", 4, 4, 48)], 49),
    # a 2 x 2 source: every tap clamps somewhere
    "2x2-nv12": case("bgra", 23, 15, [L("img_nv12_bgra", 2, 2, 50)], 51),
    "2x2-rgba": case("bgra", 23, 15, [L("img_rgba_bgra_tx", 2, 2, 52)], 53),
    "2x2-420": case("nv12", 26, 18, [L("img_y420p_nv12", 2, 2, 54)], 55),
    # the Metal kernel: nearest, per-pixel alpha, no geometry
    "metal-up": case("bgra", 25, 17, [L("img_bgra_bgra", 11, 8, 56)], 57),
    "metal-down": case("bgra", 25, 17, [L("img_bgra_bgra", 61, 40, 58)], 59),
    # mixed stacks on cleared canvases
    "stack-bgra": case("bgra", 52, 34, [L("img_nv12_bgra", 41, 27, 60), L("img_rgba_bgra_tx", 20, 14, 61, rect=(5.5, 4.5, 22.0, 15.0), opacity=0.8),
                                        L("img_y420p_bgra", 24, 18, 62, csc=1, rect=(28.3, 15.4, 30.2, 25.1), opacity=0.45),
                                        L("img_bgra_bgra_tx", 16, 10, 63, rect=(20.0, 2.0, 15.0, 9.0), rotation=0.3)]),
    "stack-nv12": case("nv12", 52, 34, [L("img_nv12_nv12", 41, 27, 64), L("img_y420p_nv12", 20, 14, 65, rect=(5.5, 4.5, 22.0, 15.0), opacity=0.8),
                                        L("img_bgra_nv12_int", 24, 18, 66, rect=(28.3, 15.4, 30.2, 25.1)),
                                        L("img_rgba_nv12_int", 16, 10, 67, csc=1, rect=(20.0, 2.0, 15.0, 9.0), opacity=0.4)]),
    "stack-y420p": case("y420p", 52, 34, [L("img_y420p_y420p", 41, 27, 68), L("img_bgra_y420p_int", 20, 14, 69, rect=(5.5, 4.5, 22.0, 15.0)),
                                          L("img_y420p_y420p", 24, 18, 70, rect=(28.3, 15.4, 30.2, 25.1), opacity=0.45)]),
    # the float RGB -> YUV kernels (the statement's "premul" family), at the sizes of their _int neighbours
    "up-premul": case("y420p", 30, 18, [L("img_bgra_y420p", 13, 9, 400)], 401),
    "down-premul": case("nv12", 22, 14, [L("img_rgba_nv12", 61, 47, 402, opacity=0.6519)], 403),
    "left-top-premul": case("nv12", 40, 26, [L("img_bgra_nv12", 30, 20, 404, rect=(-9.3, -5.7, 31.1, 20.9))], 405),
    "right-bottom-premul": case("y420p", 40, 26, [L("img_rgba_y420p", 30, 20, 406, rect=(20.6, 12.2, 33.3, 25.1))], 407),
    "rotated-premul": case("nv12", 48, 30, [L("img_rgba_nv12", 40, 24, 408, rect=(12.0, 7.0, 26.0, 15.0), rotation=2.4)], 409),
    "border-fill-premul": case("y420p", 44, 28, [L("img_bgra_y420p", 24, 16, 410, rect=(9.3, 6.4, 22.1, 13.3), border=(3.2, 2.3, 4.1, 5.4),
                                                   fill=(0.2, 0.8, 0.4, 0.35), opacity=0.8137)], 411),
    "border-fill-premul-nv12": case("nv12", 44, 28, [L("img_rgba_nv12", 24, 16, 412, rect=(9.3, 6.4, 22.1, 13.3), border=(3.2, 2.3, 4.1, 5.4),
                                                        fill=(0.9, 0.3, 0.55, 0.6), opacity=0.7519)], 413),
    # a crop reaching outside [0, 1]: pixels inside tx whose uv is outside get the fill alone
    "crop-outside-premul": case("nv12", 36, 22, [L("img_bgra_nv12", 50, 30, 414, tex=(-0.15, 0.3, 1.2, 0.9), fill=(0.13, 0.27, 0.91, 0.8))], 415),
    "flip-premul": case("y420p", 36, 22, [L("img_rgba_y420p", 50, 30, 416, tex=(0.9, 0.1, -0.8, 0.8))], 417),
    "opacity-0-premul": case("nv12", 22, 14, [L("img_bgra_nv12", 14, 11, 418, opacity=0.0, fill=(1.0, 1.0, 1.0, 1.0))], 419),
    "opacity-1-premul": case("y420p", 22, 14, [L("img_bgra_y420p", 14, 11, 420, opacity=1.0)], 421),
    "odd-premul-nv12": case("nv12", 27, 15, [L("img_rgba_nv12", 21, 13, 422, rect=(-2.3, 1.2, 30.1, 15.3))], 423),
    "odd-premul-y420p": case("y420p", 15, 27, [L("img_rgba_y420p", 13, 21, 424, opacity=0.9137)], 425),
    "2x2-premul": case("nv12", 26, 18, [L("img_bgra_nv12", 2, 2, 426)], 427),
    # two of them over a video layer on a cleared canvas: per-pixel alpha through re-quantised layers; and a mix on a seeded canvas
    "stack-premul-video": case("y420p", 52, 34, [L("img_y420p_y420p", 41, 27, 428), L("img_bgra_y420p", 20, 14, 429, rect=(5.5, 4.5, 32.0, 20.0), opacity=0.8137),
                                                 L("img_rgba_y420p", 24, 18, 430, rect=(18.3, 10.4, 30.2, 21.1), opacity=0.4519)]),
    "stack-premul-seeded": case("nv12", 52, 34, [L("img_bgra_nv12", 41, 27, 431, opacity=0.7137), L("img_rgba_nv12_int", 20, 14, 432, rect=(5.5, 4.5, 22.0, 15.0)),
                                                 L("img_rgba_nv12", 24, 18, 433, rect=(20.3, 9.4, 30.2, 22.1), fill=(0.3, 0.6, 0.1, 0.5), border=(2.2, 1.3, 2.1, 1.4))], 434),
}
# identity placement on texel centres: a 2^k canvas, a source of the same size moved by half a texel (1 / 2^(k+1) is exact), so that every tap
# position is an integer and every weight 0 or 1: EVERY byte must be decided, and equal to the source's
IDENTITY = {
    "identity-nv12": case("bgra", 16, 8, [L("img_nv12_bgra", 16, 8, 80, tex=(-1.0 / 32, -1.0 / 16, 1.0, 1.0))], 81),
    "identity-bgra": case("bgra", 16, 8, [L("img_bgra_bgra_tx", 16, 8, 82, tex=(-1.0 / 32, -1.0 / 16, 1.0, 1.0))], 83),
    "identity-int": case("y420p", 16, 8, [L("img_rgba_y420p_int", 16, 8, 86, tex=(-1.0 / 32, -1.0 / 16, 1.0, 1.0))], 87),
    # the plain full-canvas layer of the same size: taps half way between texels, all weights 1/4: exact in f32, ties included
    "identity-box-bgra": case("bgra", 16, 8, [L("img_y420p_bgra", 16, 8, 88)], 89),
}
NAMED.update(IDENTITY)
# (the reference's 4:2:0 kernels have no such case for chroma: luma and chroma taps of one uv lie half a chroma sample apart, and their unit-scale
# chain rounds at c / 255 whatever the weights are.  The luma plane of this one is decided and equals the source's.)
NAMED["aligned-luma-420"] = case("nv12", 16, 8, [L("img_nv12_nv12", 16, 8, 84, tex=(-1.0 / 32, -1.0 / 16, 1.0, 1.0))], 85)


# ---- b. seeded cases in the style of the fuzzers' _random_case -------------------------------------------------------------------------------------
def random_case(seed, yuv_kernels=YUV_KERNELS):
    """rectangles across edges, rotation, borders, fill, texture crop and flip, opacity in {0, 1, random}; 1 - 4 layers; every third canvas cleared"""
    rng = np.random.default_rng(seed)
    fmt = ["bgra", "nv12", "bgra", "y420p"][seed % 4]
    W, H = int(rng.integers(8, 150)), int(rng.integers(8, 90))
    names = BGRA_KERNELS if fmt == "bgra" else yuv_kernels[fmt]
    layers = []
    for _ in range(int(rng.integers(1, 5))):
        kw = {}
        if rng.random() < 0.8:
            kw["rect"] = (float(rng.uniform(-0.4, 0.8) * W), float(rng.uniform(-0.4, 0.8) * H), float(rng.uniform(0.1, 1.6) * W), float(rng.uniform(0.1, 1.6) * H))
        if rng.random() < 0.4:
            kw["rotation"] = float(rng.uniform(-3.2, 3.2))
        if rng.random() < 0.5:
            kw["border"] = tuple(float(v) for v in rng.uniform(0, 12, 4))
        if rng.random() < 0.5:
            kw["fill"] = tuple(float(v) for v in rng.uniform(0, 1, 4))
        if rng.random() < 0.5:
            kw["tex"] = (float(rng.uniform(-0.2, 0.5)), float(rng.uniform(-0.2, 0.5)), float(rng.uniform(0.2, 1.3)) * (1 if rng.random() < 0.8 else -1),
                         float(rng.uniform(0.2, 1.3)))
        kw["opacity"] = float(rng.choice([1.0, 0.0, rng.uniform(0, 1)]))
        layers.append(L(names[int(rng.integers(0, len(names)))], int(rng.integers(2, 200)), int(rng.integers(2, 120)), int(rng.integers(1, 1 << 20)),
                        csc=int(rng.integers(0, 4)), **kw))
    return case(fmt, W, H, layers, None if seed % 3 == 0 else 7000 + seed)


# ---- the shapes of tests/test_gpu_composite_f64.py: no larger than the smallest at which a route is eligible and has more than one strip, chunk
# or wave.  Pictures are placed by rectangles with fractional corners: tap positions that are no dyadic rationals, and no rounding tie every
# other pixel as 480 -> 320 on the pixel grid would have; opacities are no short decimals: p 0.35 + cur 0.65 is a tie for one (p, cur) in twenty
FR = dict(rect=(-3.3, -2.7, 327.1, 186.9))           # covers a 320 x 180 canvas
FR_INT = dict(rect=(-2.3, -1.7, 261.1, 99.9))        # covers a 256 x 96 canvas
FR_PH = dict(rect=(-1.3, -1.1, 131.2, 98.9), content="waves")         # covers a 128 x 96 canvas


def _stack(kernel, iw, ih, seed, ops, cscs, **kw):
    return [L(kernel, iw, ih, seed + i, csc=c, opacity=o, **kw) for i, (o, c) in enumerate(zip(ops, cscs))]


ROUTES = {
    # tick_bgra_stream: 1 - 4 layers of one geometry on a cleared canvas, opaque and translucent bottoms, NV12 and y420p
    "st-nv12-4": case("bgra", 320, 180, _stack("img_nv12_bgra", 480, 270, 200, (1.0, 0.7137, 0.4519, 0.2283), (0, 1, 3, 2), **FR)),
    "st-nv12-2t": case("bgra", 320, 180, _stack("img_nv12_bgra", 480, 270, 210, (0.6137, 0.3519), (1, 0), content="waves", **FR)),
    "st-nv12-1": case("bgra", 320, 180, _stack("img_nv12_bgra", 480, 270, 220, (1.0,), (3,), content="waves", **FR)),
    "st-y420p-3": case("bgra", 320, 180, _stack("img_y420p_bgra", 480, 270, 230, (1.0, 0.5531, 0.3127), (2, 0, 1), **FR)),
    "st-y420p-2t": case("bgra", 320, 180, _stack("img_y420p_bgra", 480, 270, 235, (0.8093, 0.4177), (3, 1), content="waves", **FR)),
    "st-y420p-1": case("bgra", 320, 180, _stack("img_y420p_bgra", 480, 270, 240, (0.8093,), (1,), content="waves", **FR)),
    # one batch planned in phases: five ticks of four layers
    **{f"ph{t}": case("bgra", 128, 96, _stack("img_nv12_bgra", 192, 144, 250 + 10 * t, (1.0, 0.7137, 0.4519, 0.2283), (0, 1, 3, 0), **FR_PH)) for t in range(5)},
    # tick_bgra_wave / tick_general_bgra: every source class, across the edges, border and fill, a texture window, on a seeded canvas
    "wv-mix": case("bgra", 260, 70, [L("img_y420p_bgra", 96, 54, 300, csc=1, rect=(0.4, 0.3, 130.3, 69.2)),
                                     L("img_nv12_bgra", 96, 54, 301, rect=(130.6, 0.2, 129.1, 69.5), opacity=0.9),
                                     L("img_rgba_bgra_tx", 50, 40, 302, rect=(-20.3, -10.2, 120.4, 60.7), fill=(0.1, 0.5, 0.9, 0.8), opacity=0.35),
                                     L("img_bgra_bgra_tx", 33, 17, 303, rect=(150.2, 5.3, 90.4, 60.1), tex=(0.25, 0.0, 0.5, 1.0), fill=(0.93, 0.88, 0.07, 0.9))], 304),
    "wv-cover": case("bgra", 200, 70, [L("img_bgra_bgra_tx", 200, 70, 310, opacity=0.7, rect=(-1.2, -0.7, 203.1, 72.3)),
                                       L("img_nv12_bgra", 300, 106, 311, csc=2, opacity=0.6, rect=(-1.2, -0.7, 203.1, 72.3))], 312),
    # the Metal kernel's layer (nearest, no geometry) over a video: applied per pixel inside the strip kernel
    "wv-metal": case("bgra", 200, 70, [L("img_nv12_bgra", 300, 106, 380, csc=1, rect=(-1.2, -0.7, 203.1, 72.3)), L("img_bgra_bgra", 123, 41, 381)], 382),
    # tick_yuv_stream / tick_yuv_wave / tick_general_yuv: video layers, the integer-matrix encoder rows
    "ys-nv12-video": case("nv12", 320, 180, [L("img_nv12_nv12", 480, 270, 320, **FR),
                                             L("img_y420p_nv12", 160, 64, 321, rect=(120.4, 20.3, 160.2, 64.1), opacity=0.55)]),
    "ys-y420p-video": case("y420p", 320, 180, [L("img_y420p_y420p", 480, 270, 330, opacity=0.8, **FR)]),
    "ys-nv12-int": case("nv12", 256, 96, [L("img_bgra_nv12_int", 256, 96, 340, csc=1, **FR_INT),
                                          L("img_rgba_nv12_int", 64, 36, 341, csc=2, rect=(30.4, 10.3, 80.1, 45.2), opacity=0.8)]),
    "ys-y420p-int": case("y420p", 256, 96, [L("img_rgba_y420p_int", 256, 96, 350, csc=3, opacity=0.9, **FR_INT),
                                            L("img_bgra_y420p_int", 96, 54, 351, rect=(100.2, 20.6, 120.3, 70.4), opacity=0.6, border=(4.2, 4.1, 4.3, 4.4))]),
    # the strip kernel only: fill paint, a flip, an uncleared canvas
    "yw-nv12-mix": case("nv12", 260, 70, [L("img_y420p_nv12", 96, 54, 360, rect=(33.3, 9.4, 180.2, 40.1), border=(5.2, 3.1, 7.3, 2.4), fill=(0.9, 0.2, 0.1, 0.6), opacity=0.8),
                                          L("img_nv12_nv12", 64, 64, 361, rect=(150.2, 5.3, 90.4, 60.1), tex=(1.0, 0.0, -1.0, 1.0), opacity=0.7),
                                          L("img_rgba_nv12_int", 50, 40, 362, rect=(-20.3, -10.2, 120.4, 60.7), opacity=0.35)], 363),
    "yw-y420p-mix": case("y420p", 192, 108, [L("img_y420p_y420p", 192, 108, 370, rect=(-1.2, -0.7, 195.1, 110.3)),
                                             L("img_bgra_y420p_int", 64, 36, 371, csc=1, rect=(8.3, 8.4, 64.2, 36.1), opacity=0.8, fill=(0.2, 0.9, 0.1, 0.45))], 372),
    # the float RGB -> YUV rows of tick_yuv_stream / tick_yuv_wave, per canvas format: float RGB layers only; a video layer with two of them
    # over it (the three-layer instantiation of own | RGB kinds); a video, a float RGB and an integer-matrix layer in four (the all-kinds one)
    **{f"ys-{fmt}-rgb": case(fmt, 256, 96, [L(f"img_bgra_{fmt}", 256, 96, 500 + s, opacity=0.9137, **FR_INT),
                                            L(f"img_rgba_{fmt}", 64, 36, 501 + s, rect=(30.4, 10.3, 80.1, 45.2), opacity=0.8137)])
       for fmt, s in (("nv12", 0), ("y420p", 40))},
    **{f"ys-{fmt}-rgb3": case(fmt, 256, 96, [L(f"img_{fmt}_{fmt}", 384, 144, 510 + s, content="waves", **FR_INT),
                                             L(f"img_bgra_{fmt}", 96, 54, 511 + s, rect=(100.2, 20.6, 120.3, 70.4), opacity=0.6137, border=(4.2, 4.1, 4.3, 4.4)),
                                             L(f"img_rgba_{fmt}", 64, 36, 512 + s, rect=(30.4, 10.3, 80.1, 45.2), opacity=0.8137)])
       for fmt, s in (("nv12", 0), ("y420p", 40))},
    **{f"ys-{fmt}-all4": case(fmt, 256, 96, [L(f"img_y420p_{fmt}", 384, 144, 520 + s, content="waves", **FR_INT),
                                             L(f"img_rgba_{fmt}", 64, 36, 521 + s, rect=(30.4, 10.3, 80.1, 45.2), opacity=0.8137),
                                             L(f"img_bgra_{fmt}_int", 96, 54, 522 + s, csc=1, rect=(100.2, 20.6, 120.3, 70.4), opacity=0.6137),
                                             L(f"img_bgra_{fmt}", 48, 32, 523 + s, rect=(180.3, 40.2, 70.4, 50.1), opacity=0.7519)])
       for fmt, s in (("nv12", 0), ("y420p", 40))},
    # the strip kernel only: border and fill, a flip, a layer across the left and top edges, an uncleared canvas — the edge strips go through the
    # per-pixel statement of yuv_pixel.hip.h, the interior through the row code
    "yw-nv12-premul": case("nv12", 260, 70, [L("img_nv12_nv12", 96, 54, 530, rect=(33.3, 9.4, 180.2, 40.1), opacity=0.8137),
                                             L("img_bgra_nv12", 64, 64, 531, rect=(150.2, 5.3, 90.4, 60.1), tex=(1.0, 0.0, -1.0, 1.0), opacity=0.7137,
                                               border=(5.2, 3.1, 7.3, 2.4), fill=(0.9, 0.2, 0.1, 0.6)),
                                             L("img_rgba_nv12", 50, 40, 532, rect=(-20.3, -10.2, 120.4, 60.7), opacity=0.3519)], 533),
    "yw-y420p-premul": case("y420p", 192, 108, [L("img_rgba_y420p", 192, 108, 570, rect=(-1.2, -0.7, 195.1, 110.3), opacity=0.9137),
                                                L("img_bgra_y420p", 64, 36, 571, rect=(8.3, 8.4, 64.2, 36.1), opacity=0.8137, fill=(0.2, 0.9, 0.1, 0.45),
                                                  border=(3.1, 2.2, 4.3, 2.4)),
                                                L("img_rgba_y420p", 48, 30, 572, rect=(-10.3, -6.2, 80.4, 50.7), tex=(1.0, 0.0, -1.0, 1.0), opacity=0.5519)], 573),
}

# literal seeds, chosen when the list was written from 100 ... 169 by the statement alone: one whose tick leaves nine tenths of the canvas as it
# was (opacity 0, a picture off the canvas: a third of the generator's draws) or whose statement exceeds a cap was left out; none is skipped at
# run time, and both conditions are asserted below
SEEDS = [104, 105, 106, 108, 109, 110, 111, 112, 114, 116, 118, 121, 123, 124, 126, 127, 128, 129, 134, 135, 136, 138, 139, 140, 141, 142, 143, 144,
         146, 147, 148, 149, 150, 151, 152, 154, 155, 156, 157, 158, 160, 161, 162, 163, 166, 167, 168, 169]
SEEDED = {f"seed{s}": random_case(s) for s in SEEDS}
# the float RGB -> YUV kernels: the same generator drawing from PREMUL_KERNELS.  Literal seeds, chosen the same way from the odd numbers from 201
# on (s % 4 == 1: NV12, 3: y420p), sixteen of each format: left out were the no-ops and the draws without one of the four kernels; none of
# these exceeded a cap.  Both conditions are asserted below as well
SEEDS_PREMUL = [205, 217, 221, 229, 245, 249, 253, 257, 261, 265, 269, 273, 281, 289, 297, 301,
                203, 215, 219, 223, 235, 243, 247, 251, 255, 263, 267, 271, 275, 279, 283, 287]
SEEDED_PREMUL = {f"premul-seed{s}": random_case(s, PREMUL_KERNELS) for s in SEEDS_PREMUL}
CASES = {**NAMED, **SEEDED, **SEEDED_PREMUL, **ROUTES}


def waves(noise, seed):
    """a plane of the same shape: a sine surface of amplitude 90 with the low five bits of the seeded noise on top — neighbouring texels differ by
    about 35 codes at most where seeded noise differs by up to 255, and the position term of the bound scales with that difference: a video
    layer 480 -> 327 leaves 0.2 - 0.3 % of its bytes open on this content, about 2.3 % on noise.  The deepest stacks of the route shapes keep
    noise, the others take this, so that the module's pool stays well under its cap"""
    h, w = noise.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    comps = 1 if noise.ndim == 2 else noise.shape[2]
    phase = seed % 7 + 1.3 * np.arange(comps)
    v = 128.0 + 90.0 * np.sin(2.0 * np.pi * (1.3 * x / w + 0.7 * y / h)[..., None] + phase)
    v = v[..., 0] if noise.ndim == 2 else v
    return np.ascontiguousarray((np.rint(v).astype(np.int64) - 16 + (noise & 31)).clip(0, 255).astype(np.uint8))


# ---- building a case ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(name):
    """(canvas planes before the tick, [(kernel, source planes, uniforms, colourspace)]), read-only"""
    fmt, W, H, canvas_seed, layers = CASES[name]
    planes = util.alloc_image(fmt, W, H, seed=1 if canvas_seed is None else canvas_seed)
    out = []
    for kernel, iw, ih, seed, csc, kw in layers:
        kw = dict(kw)
        src = util.alloc_image(F.KERNELS[kernel][0], iw, ih, seed=seed)
        if kw.pop("content", "noise") == "waves":
            src = [waves(p, seed + k) for k, p in enumerate(src)]
        for p in src:
            p.setflags(write=False)
        out.append((kernel, src, util.make_uniforms((W, H), in_size=(iw, ih), **dict(kw)), csc))
    for p in planes:
        p.setflags(write=False)
    return planes, out


@functools.lru_cache(maxsize=None)
def statement(name):
    """the float64 intervals of a case, computed once and shared (read-only)"""
    fmt, W, H, canvas_seed, _ = CASES[name]
    planes, layers = build(name)
    canvas = F.tick(fmt, W, H, planes, canvas_seed is None, layers)
    for lo, hi in canvas:
        lo.setflags(write=False)
        hi.setflags(write=False)
    return canvas


@functools.lru_cache(maxsize=None)
def oracle(name):
    fmt, W, H, canvas_seed, _ = CASES[name]
    planes, layers = build(name)
    exp = util.copy_image(planes)
    if canvas_seed is None:
        assert O.run_kernel(f"img_clear_{fmt}", exp) == 0
    for kernel, src, u, csc in layers:
        assert O.run_kernel(kernel, exp, src, u, csc=csc) == 0
    return exp


def changed(name):
    """the share of the canvas's bytes that the tick must change, by the statement (a cleared canvas counts from its clear values)"""
    fmt, W, H, canvas_seed, _ = CASES[name]
    before = F.tick(fmt, W, H, build(name)[0], canvas_seed is None, [])
    return sum(int(((lo > b) | (hi < b)).sum()) for (lo, hi), (b, _) in zip(statement(name), before)) / sum(b.size for b, _ in before)


def within(name, got, what):
    for i, ((lo, hi), g) in enumerate(zip(statement(name), got)):
        assert_within(lo, hi, g, f"{what}: {name} plane {i}")


def outside(canvas, got):
    """the share of bytes outside their interval, and the share more than 8 codes outside"""
    n = bad = far = 0
    for (lo, hi), g in zip(canvas, got):
        g = np.asarray(g).astype(np.int64)
        d = np.maximum(lo - g, g - hi)
        n, bad, far = n + g.size, bad + int((d > 0).sum()), far + int((d > 8).sum())
    return bad / n, far / n


def test_every_kernel_is_covered_singly_and_in_stacks():
    single = {c[4][0][0] for c in CASES.values() if len(c[4]) == 1}
    stacked = {l[0] for c in CASES.values() if len(c[4]) > 1 for l in c[4]}
    assert single == set(F.KERNELS), set(F.KERNELS) - single
    assert stacked >= set(F.KERNELS) - {"img_bgra_bgra"}, set(F.KERNELS) - stacked
    assert {len(c[4]) for c in CASES.values()} >= {1, 2, 3, 4}
    assert {c[3] is None for c in CASES.values()} == {True, False}
    assert len(SEEDED) >= 40 and all(changed(name) >= 0.10 for name in SEEDED)
    assert len(SEEDED_PREMUL) >= 24 and all(changed(name) >= 0.10 for name in SEEDED_PREMUL)
    assert [c[0] for c in SEEDED_PREMUL.values()].count("nv12") == [c[0] for c in SEEDED_PREMUL.values()].count("y420p") == len(SEEDED_PREMUL) // 2
    assert all(any(F.KERNELS[l[0]][2] == "premul" for l in c[4]) for c in SEEDED_PREMUL.values())
    for fmt, W, H, _, layers in NAMED.values():
        assert 7 <= W <= 150 and 5 <= H <= 90
    for fmt, W, H, _, layers in CASES.values():
        for kernel, iw, ih, seed, csc, kw in layers:
            kw = dict(kw)
            assert kw.pop("content", "noise") in ("noise", "waves")
            assert iw <= 512 and 0.0 <= kw.get("opacity", 1.0) <= 1.0 and all(0.0 <= f <= 1.0 for f in kw.get("fill", ())), "the statement's scope"


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_lies_within_the_statement(name):
    within(name, oracle(name), "oracle")


@pytest.mark.parametrize("name", list(IDENTITY))
def test_identity_placement_is_decided_everywhere(name):
    for lo, hi in statement(name):
        assert np.array_equal(lo, hi)
    planes, ((kernel, src, u, csc),) = build(name)
    if kernel == "img_bgra_bgra_tx":        # alpha 255 texels come through unchanged; the others are blended with the canvas
        lo = statement(name)[0][0]
        opaque = src[0][..., 3] == 255
        assert np.array_equal(lo[opaque][:, :3], src[0][opaque][:, :3])


def test_aligned_luma_of_a_420_canvas_is_decided():
    lo, hi = statement("aligned-luma-420")[0]
    assert np.array_equal(lo, hi) and np.array_equal(lo, build("aligned-luma-420")[1][0][1][0])


# ---- d. the caps, from the statement alone -------------------------------------------------------------------------------------------------------
def test_caps_per_case_and_pooled():
    caps = F.Caps()
    for name in CASES:
        caps.add(statement(name), name)
    caps.assert_pool("named and seeded cases")


# ---- c. wrong statements are caught ---------------------------------------------------------------------------------------------------------------
WRONG = {
    "pixel-centred out_uv": (dict(out_uv=lambda x, size: (x + 0.5, size)), ["up-nv12", "down-rgba", "flip-420"]),
    "a and 1 - a exchanged": (dict(blend=lambda p, a, cur: p * (1.0 - a) + cur * a), ["opacity-frac", "opacity-frac-420", "alpha-stack"]),
    "no RGBA swizzle": (dict(swizzle=False), ["down-rgba", "flip-int", "left-top-premul"]),
    "chroma sampled at luma texel coordinates": (dict(chroma_size=lambda plane_wh, luma_wh: luma_wh), ["up-nv12", "down-y420p", "flip-420"]),
    "a = sample_A opacity without / 255": (dict(alpha_scale=1.0), ["up-bgra", "alpha-stack-int"]),
    "chroma owned by the odd pixel of the quad": (dict(chroma_owner=1), ["flip-420", "up-int", "odd-y420p", "up-premul"]),
    "floor replaced by round in the tap index": (dict(tap_index=np.round), ["up-nv12", "up-bgra", "opacity-frac-420"]),
    # the float RGB -> YUV kernels
    "colours not multiplied by their alpha before the matrix": (dict(premul=lambda c, a: c), ["up-premul", "border-fill-premul-nv12", "stack-premul-video"]),
    "the fill painted everywhere inside the border quad": (dict(fill_inside="border"), ["border-fill-premul", "border-fill-premul-nv12"]),
    "the matrix offset added outside the blend": (dict(offset_blended=False), ["down-premul", "flip-premul"]),
}


@pytest.mark.parametrize("what", list(WRONG))
def test_a_wrong_statement_fails(what):
    """far outside: at least 5 % of a case's bytes leave the wrong statement's intervals (the right one holds all of them: test above)"""
    how, names = WRONG[what]
    for name in names:
        fmt, W, H, canvas_seed, _ = CASES[name]
        planes, layers = build(name)
        bad, far = outside(F.tick(fmt, W, H, planes, canvas_seed is None, layers, **how), oracle(name))
        print(f"wrong: {what}: {name}: {100 * bad:.1f} % outside, {100 * far:.1f} % by more than 8 codes")
        assert bad > 0.05, (what, name, bad)
