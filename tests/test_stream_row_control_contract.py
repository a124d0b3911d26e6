"""The row loop of tick_bgra_stream on the built gfx950 object: what was taken out of a row's control stays out, and the tap reads the
kernel issues by hand are not touched while they are in flight.  Reads `kernels_stream.hip.o` like tests/test_device_code_contract.py
(skipped where the objects are not built); no GPU needed.

Counted with tools/row_loop_count.py over the whole row loop (the kernel's outermost loop: row body, ring logic, request loops and the
row-table refill, every path together), four layers, absorbed colour matrix, hipcc 7.2:

                                  s_waitcnt lgkmcnt   SALU   VALU   LDS
    before (a wait per tap)   NV12       47            152    212    52
                              y420p      46            153    214    52
    one wait per layer        NV12        8            158    215    52
                              y420p       8            157    214    52

The bounds are the shipped counts plus 2 for the compiler's freedom.  (The SALU bound only holds the line: the scalar instructions of
the ring logic measured as free on the GPU — profiles/stream_row_control_notes.md — and were left as they are.)"""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
OBJ = ROOT / "swiftvideo_amd" / "csrc" / "kernels_stream.hip.o"
sys.path.insert(0, str(ROOT / "tools"))
import row_loop_count  # noqa: E402

LGKM_WAITS_MAX = 8 + 2
SALU_MAX = 158 + 2


@pytest.fixture(scope="module")
def stream_kernels(tmp_path_factory):
    if not OBJ.exists() or not (row_loop_count.LLVM / "llvm-objcopy").exists():
        pytest.skip(f"{OBJ.name} not built here")
    return row_loop_count.kernels(row_loop_count.code_object(OBJ, tmp_path_factory.mktemp("stream_co")), prefix="_ZN3chv")


@pytest.mark.parametrize("inst", ["ILi4ELb0ELb1E", "ILi4ELb1ELb1E"], ids=["nv12", "y420p"])
def test_row_loop_keeps_one_wait_per_layer(stream_kernels, inst):
    name = "_ZN3chv16tick_bgra_stream" + inst
    hits = {n: i for n, i in stream_kernels.items() if n.startswith(name)}
    assert len(hits) == 1, sorted(stream_kernels)[:4]
    loop = row_loop_count.row_loop(next(iter(hits.values())))
    c = row_loop_count.classes(loop)
    print(inst, c)
    assert sum(1 for _, op, _ in loop if op == "v_fma_mix_f32") == 60, "not the row loop"
    assert c["lds"] >= 48 + 2                                     # 48 taps + the row entry: the taps are still byte reads
    assert c["lgkm_waits"] <= LGKM_WAITS_MAX, c
    assert c["salu"] <= SALU_MAX, c


def _regs(operand):
    """VGPR numbers an operand names: v7, v[4:7]"""
    out = set()
    for m in re.finditer(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]", operand):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def inflight_violations(ins):
    """Walk a kernel in address order: every LDS read's destination is in flight until an `s_waitcnt lgkmcnt(n)` leaves at most n younger
    LDS operations outstanding (LDS operations of a wave complete in order; scalar loads, which complete out of order, conservatively
    drain nothing here and are drained only by lgkmcnt(0)).  Any instruction that names an in-flight register is a violation.  Control flow
    is ignored: the kernel issues and awaits a group inside one basic block, and a branch target that inherits reads in flight is itself
    reported because the walk keeps them in flight across it."""
    pending, bad = [], []        # [(set of destination registers)] in issue order
    for addr, op, args in ins:
        if op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", args)
            if m:
                n = int(m.group(1))
                pending = pending[len(pending) - n:] if n else []
            continue
        named = _regs(args)
        flying = set().union(*pending) if pending else set()
        if named & flying:
            bad.append((hex(addr), op, args, sorted(named & flying)))
        if op.startswith("ds_read"):
            pending.append(_regs(args.split(",")[0]))
        elif op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load"):
            pending.append(set())
    return bad


def test_hand_issued_tap_reads_are_not_touched_in_flight(stream_kernels):
    """st_taps_read issues a layer's twelve byte reads from an asm statement; hipcc believes their destinations written when the statement
    ends.  Between a read and the wait that covers it no instruction may read, copy, spill or overwrite a destination — in every
    instantiation of the streaming kernels (1 - 4 layers, NV12 and planar, both matrix forms, batch and lone-tick twins)."""
    seen = 0
    for name, ins in stream_kernels.items():
        if "tick_bgra_stream" not in name:
            continue
        seen += 1
        assert sum(1 for _, op, _ in ins if op == "ds_read_u8") >= 12, name
        bad = inflight_violations(ins)
        assert not bad, (name, bad[:4])
    assert seen == 32, seen


def test_inflight_check_sees_a_violation():
    """the walker itself: a consumer in front of the wait, a copy of a destination, a wait that leaves the read outstanding"""
    ok = [(0, "ds_read_u8", "v1, v9"), (4, "ds_read_u8", "v2, v9 offset:1"), (8, "s_waitcnt", "lgkmcnt(1)"), (12, "v_add_u32_e32", "v3, v1, v1"),
          (16, "s_waitcnt", "lgkmcnt(0)"), (20, "v_add_u32_e32", "v3, v2, v2")]
    assert inflight_violations(ok) == []
    early = [(0, "ds_read_u8", "v1, v9"), (4, "v_fma_mix_f32", "v3, v4, v1, 0"), (8, "s_waitcnt", "lgkmcnt(0)")]
    assert inflight_violations(early)
    copy = [(0, "ds_read_u8", "v1, v9"), (4, "v_mov_b32_e32", "v5, v1"), (8, "s_waitcnt", "lgkmcnt(0)")]
    assert inflight_violations(copy)
    short = [(0, "ds_read_u8", "v1, v9"), (4, "ds_read_u8", "v2, v9"), (8, "s_waitcnt", "lgkmcnt(1)"), (12, "v_mov_b32_e32", "v5, v2")]
    assert inflight_violations(short)
    wide = [(0, "ds_read_b128", "v[4:7], v9"), (4, "v_mov_b32_e32", "v0, v6"), (8, "s_waitcnt", "lgkmcnt(0)")]
    assert inflight_violations(wide)
