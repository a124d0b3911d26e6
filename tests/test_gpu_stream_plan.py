"""tick_bgra_stream's launch plan (swiftvideo_amd/csrc/stream_plan.h): a batch cut into phases of falling chunk heights — tall chunks over the
first ticks, short ones over the last — must write the bytes the uniform launch writes.  CHV_STREAM_PLAN=N plans as if the chip held N
waves (and a tenth of a round in the tall phase were enough), so that batches of 5 and 13 small ticks (phase sizes that are no multiple
of 8 blocks) get several phases: at N = 40 the tall phase takes the 96-row canvas in one chunk, across two refills of the 32-row table,
and the closing phases halve it (96 / 48 / 24); at N = 160 five ticks are too few for that and are cut 48 / 24, thirteen still 96 / 48 / 24.
Thirteen ticks on a 192-row canvas get four phases (192 / 96 / 48 / 24: every branch of the kernels' phase search).  Every kernel family the plan is threaded
through runs: the f32-tap kernels, the chroma-carry kernels (CHV_STREAM_F32TAPS=0), the opaque-bottom kernels (planar sources) and the
general ones (a bottom layer that is not opaque).  Every canvas — pre-filled with seeded garbage, so that a row no wave covers shows — is
compared byte for byte with the oracle, phased (`stream_phased_launches` must move) and with CHV_STREAM_PLAN=0 (it must not)."""
import pytest

import gpuutil as G
import util
from oracle import oracle as O
from swiftvideo_amd import chipvideo as cv
from swiftvideo_amd import compute as sv

pytestmark = pytest.mark.gpu

STREAM = "tick_bgra_stream"
PHASED, F32, CARRY, OPAQUE = "stream_phased_launches", "stream_f32tap_launches", "stream_carry_launches", "stream_opaque_launches"
CANVAS = (128, 96)
SOURCES = [(128, 144), (192, 144)]           # 1.5 : 1 down; the same with 1.5 : 1 across as well (every lane's taps differ from its neighbour's)
FAMILIES = {
    # format, opacities, CHV_STREAM_F32TAPS, the counters that must move
    "f32taps4": ("nv12", (1.0, 0.75, 0.5, 0.25), "1", (F32, CARRY, OPAQUE)),
    "f32taps2": ("nv12", (1.0, 0.5), "1", (F32, CARRY, OPAQUE)),
    "carry4": ("nv12", (1.0, 0.75, 0.5, 0.25), "0", (CARRY, OPAQUE)),
    "carry2": ("nv12", (1.0, 0.5), "0", (CARRY, OPAQUE)),
    "opaque3": ("y420p", (1.0, 0.6, 0.3), "1", (OPAQUE,)),
    "general3": ("nv12", (0.6, 0.5, 0.3), "1", ()),
}
ABSORBED = [0, 1, 3]
PLANS = ["40", "160", "0"]


def _tick(ctx, fmt, canvas, src_size, ops, seed):
    """(expected canvas by the oracle, the tick's layers on the device)"""
    (cw, ch), (sw, sh) = canvas, src_size
    exp = util.alloc_image("bgra", cw, ch)
    assert O.run_kernel("img_clear_bgra", exp) == 0
    layers = []
    for i, op in enumerate(ops):
        u = util.make_uniforms((cw, ch), in_size=(sw, sh), opacity=op)
        src = util.alloc_image(fmt, sw, sh, seed=seed + 7 * i)
        csc = ABSORBED[(seed + i) % 3]
        assert O.run_kernel(f"img_{fmt}_bgra", exp, src, u, csc=csc, threads=8) == 0
        layers.append((sv.defaultComputeKernelFromString(f"img_{fmt}_bgra"), G.to_gpu(ctx, fmt, sw, sh, src), u, csc))
    return exp, layers


def _run_plans(ctx, switch, family, ticks):
    """`ticks`: [(canvas size, expected, layers)] — one batch per plan setting, each on fresh garbage canvases"""
    fmt, ops, f32taps, moved = FAMILIES[family]
    switch("CHV_BGRA_PATH", "stream")
    switch("CHV_STREAM_F32TAPS", f32taps)
    for plan in PLANS:
        switch("CHV_STREAM_PLAN", plan)
        before = {c: cv.get_counter(c) for c in (PHASED, F32, CARRY, OPAQUE)}
        batch = [(G.to_gpu(ctx, "bgra", cw, ch, util.alloc_image("bgra", cw, ch, seed=77 + 3 * t + int(plan))), True, layers)
                 for t, ((cw, ch), _, layers) in enumerate(ticks)]
        h, name, keep = G.make_batch(ctx, batch)
        assert name == STREAM, f"dispatched to {name}"
        G.run_batch(ctx, h)
        G.destroy_batch(h)
        after = {c: cv.get_counter(c) for c in before}
        assert (after[PHASED] > before[PHASED]) == (plan != "0"), (family, plan, "phased launches", before[PHASED], after[PHASED])
        for c in (F32, CARRY, OPAQUE):
            assert (after[c] > before[c]) == (c in moved), (family, plan, c, before[c], after[c])
        for t, ((cw, ch), exp, _) in enumerate(ticks):
            G.assert_same(G.from_gpu(ctx, batch[t][0], "bgra", cw, ch), exp, f"{family}, CHV_STREAM_PLAN={plan}, tick {t} of {len(ticks)}")


@pytest.mark.parametrize("n_ticks", [5, 13])
@pytest.mark.parametrize("src", range(len(SOURCES)))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_phased_batches_match_the_oracle(ctx, switch, family, src, n_ticks):
    fmt, ops = FAMILIES[family][:2]
    seed = 12000 + 100 * sorted(FAMILIES).index(family) + 40 * src + n_ticks
    ticks = [(CANVAS,) + _tick(ctx, fmt, CANVAS, SOURCES[src], ops, seed + 31 * t) for t in range(n_ticks)]
    _run_plans(ctx, switch, family, ticks)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_four_phases_on_a_taller_canvas(ctx, switch, family):
    """13 ticks of 128 x 192: 10 in one 192-row chunk, then one tick each in 96-, 48- and 24-row chunks"""
    fmt, ops = FAMILIES[family][:2]
    seed = 14000 + 100 * sorted(FAMILIES).index(family)
    ticks = [((128, 192),) + _tick(ctx, fmt, (128, 192), (128, 288), ops, seed + 31 * t) for t in range(13)]
    _run_plans(ctx, switch, family, ticks)


@pytest.mark.parametrize("family", ["f32taps4", "general3"])
def test_a_tick_shorter_than_the_launch(ctx, switch, family):
    """one 128 x 50 canvas among 96-row ones, as the batch's last tick: it falls into the 24-row phase (both settings), whose chunk at row 48
    ends inside it and whose chunk at row 72 lies wholly below it — the phases are cut for the tallest tick, chunks below a shorter one
    write nothing"""
    fmt, ops = FAMILIES[family][:2]
    ticks = []
    for t in range(5):
        canvas, src = ((128, 50), (128, 74)) if t == 4 else (CANVAS, SOURCES[0])
        ticks.append((canvas,) + _tick(ctx, fmt, canvas, src, ops, 13000 + 31 * t))
    _run_plans(ctx, switch, family, ticks)
