"""chv_scale_lanczos_from_yuv_ladder against the independent float64 statement (tests/lanczos_f64.py) alone: nothing here is taken from the
oracle.  Every rung of every picture goes through the interval check of the pair, F.from_yuv_interval: a byte the statement decides is
compared for equality, and the share it leaves open is held under the existing cap of the matrix entries, F.MATRIX_CAP (5 %): no new number.
For these inputs (288x144 splitmix sources, seeds 900 to 902, all four colourspaces) the statement leaves 0.1 % to 0.6 % of a plane's
colour bytes open, far inside the cap; the "f64:" lines print the share per plane."""
import pytest

import gpuutil as G
import lanczos_f64 as F
from swiftvideo_amd import compute as sv
from test_gpu_lanczos_f64 import FORMATS, LADDER_RUNGS, LADDER_SRC, ORDERS, fill, from_yuv_case, packed, picture_to_gpu, source420

pytestmark = pytest.mark.gpu

SEEDS = (900, 901, 902)


@pytest.mark.parametrize("dfmt", ORDERS)
@pytest.mark.parametrize("sfmt", FORMATS)
def test_ladder_of_all_routes(ctx, sfmt, dfmt):
    """three pictures, four rungs (short strip body, the strip route's edge, the tile route, an enlargement); the colourspaces spread over the cases"""
    iw, ih = LADDER_SRC
    csc = (FORMATS.index(sfmt) + 2 * ORDERS.index(dfmt) + 1) % 4
    gs = [picture_to_gpu(ctx, sfmt, iw, ih, packed(sfmt, *source420(iw, ih, seed))) for seed in SEEDS]
    gd = [[fill(ctx, dfmt, ow, oh, seed + 7 + r) for seed in SEEDS] for r, (ow, oh) in enumerate(LADDER_RUNGS)]
    sv.usingContext(ctx, lambda c: sv.scaleLanczosFromYuvLadder(c, gd, gs, colorspace=csc))
    shares = F.Shares(F.MATRIX_CAP)
    for r, (ow, oh) in enumerate(LADDER_RUNGS):
        for i, seed in enumerate(SEEDS):
            # (from_yuv_case: alpha is 255 exactly, F.assert_within on every byte, the undecided share added, one "f64:" line per plane)
            from_yuv_case(ctx, (iw, ih, ow, oh), sfmt, dfmt, csc, shares, seed=seed, batch=G.from_gpu(ctx, gd[r][i], dfmt, ow, oh))
    shares.assert_pool(f"from_yuv ladder {sfmt}->{dfmt} csc{csc}")
