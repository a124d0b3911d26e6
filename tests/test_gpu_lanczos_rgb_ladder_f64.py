"""chv_scale_lanczos_rgb_ladder against the independent float64 statement (tests/lanczos_f64.py) alone: nothing here is taken from the oracle.
Every rung of every picture goes through the PLAIN check of a stored resample, F.assert_plain on F.Plane(src, ow, oh): |code - v| <= 0.5 +
delta for every sample of the plane.  The check leaves no sample out, so no cap is involved."""
import functools

import pytest

import gpuutil as G
import lanczos_f64 as F
from swiftvideo_amd import compute as sv
from test_gpu_lanczos_f64 import KINDS, fill, source4
from test_gpu_lanczos_rgb_ladder import RUNGS, SRC

pytestmark = pytest.mark.gpu

SEEDS = (900, 901, 902)


@functools.lru_cache(maxsize=None)
def ref(seed, kind, ow, oh):
    return F.Plane(source4(*SRC, seed, kind), ow, oh)


@pytest.mark.parametrize("kind", KINDS)
def test_ladder_of_all_routes(ctx, kind):
    """three pictures, six rungs: the short strip body, the strip route's edge, the tile route, an enlargement, two rungs whose axes differ"""
    iw, ih = SRC
    gs = [G.to_gpu(ctx, "bgra", iw, ih, [source4(iw, ih, seed, kind)]) for seed in SEEDS]
    gd = [[fill(ctx, "bgra", ow, oh, seed + 7 + r) for seed in SEEDS] for r, (ow, oh) in enumerate(RUNGS)]
    sv.usingContext(ctx, lambda c: sv.scaleLanczosRgbLadder(c, gd, gs))
    for r, (ow, oh) in enumerate(RUNGS):
        for i, seed in enumerate(SEEDS):
            got = G.from_gpu(ctx, gd[r][i], "bgra", ow, oh)[0]
            p = ref(seed, kind, ow, oh)
            worst, d = p.looseness(got)
            print("f64: rgb ladder %-6s rung %d (%dx%d) seed %d  worst %+.3e  delta %.3e" % (kind, r, ow, oh, seed, worst, d))
            F.assert_plain(p, got, f"rgb ladder {kind}, rung {r} ({ow}x{oh}), seed {seed}")
