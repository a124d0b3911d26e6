"""What the compiled unit of chv_scale_lanczos_hbd_to_420 (swiftvideo_amd/csrc/kernels_lanczos_hbd.hip.cpp, DESIGN.md sections 4.4.10, 5 and
6) must look like, from the code object's metadata and kernel names only: exactly the five kernels DESIGN names and none of the other units',
no scratch and no spill of either kind, the four strip variants inside the register budgets of their stated occupancy (five waves per SIMD
with the bodies up to 12 taps, four with all five), their hand-awaited loads untouched while in flight (tools/check_inflight.py).  Reads the
objects the build leaves in-tree (skipped when they are not there); no GPU needed."""
import subprocess
import sys
from pathlib import Path

from test_device_code_contract import LLVM, _code_object, _kernels

UNIT = "kernels_lanczos_hbd"
LADDER = "_ZN3chv18lanczos_hbd_ladderILi{}ELi{}EEEvNS_7HbdArgsE"
TILE = "_ZN3chv23lanczos_hbd_ladder_tileENS_7HbdArgsE"
SOURCES = {0: "p010", 1: "y420p10"}
# largest tap class a variant holds -> (waves per SIMD DESIGN.md section 6 states, the VGPR count that occupancy allows on gfx950)
VARIANTS = {12: (5, 96), 22: (4, 128)}
STRIPS = [LADDER.format(t, s) for t in VARIANTS for s in SOURCES]


def test_the_unit_holds_its_kernels_and_no_others(tmp_path):
    k = _kernels(_code_object(tmp_path, UNIT))
    assert sorted(k) == sorted(STRIPS + [TILE]), sorted(k)
    design = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    for name in ("lanczos_hbd_ladder<12, SRC>", "lanczos_hbd_ladder<22, SRC>", "lanczos_hbd_ladder_tile"):
        assert name in design, name


def test_the_other_units_keep_their_kernels(tmp_path):
    """the new unit includes the planar and the 4:2:0 row code: no sibling's kernels are instantiated in it, and theirs are untouched"""
    assert not any("planar_lanczos" in n or "lanczos_420_ladder" in n or "lanczos_to_420" in n or "lanczos3_" in n
                   for n in _kernels(_code_object(tmp_path, UNIT)))
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_to_420"))) == 7
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_420"))) == 5
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_planar_ladder"))) == 3


def test_no_scratch_no_spill_and_the_stated_occupancy(tmp_path):
    k = _kernels(_code_object(tmp_path, UNIT))
    for name, m in k.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    for maxt, (waves, limit) in VARIANTS.items():
        for s, what in SOURCES.items():
            m = k[LADDER.format(maxt, s)]
            assert m["vgpr_count"] <= limit, f"lanczos_hbd_ladder<{maxt}, {what}>: {m['vgpr_count']} VGPRs, {waves} waves per SIMD allow {limit}"
    assert k[TILE]["vgpr_count"] <= 64


def test_hand_awaited_loads_are_not_touched_while_in_flight(tmp_path):
    """the strip bodies issue their row loads from inline asm and wait for them with a hand-written wait: tools/check_inflight.py walks all
    four variants"""
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import check_inflight
    co = _code_object(tmp_path, UNIT)
    asm = subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    seen, bad = check_inflight.check(asm, r"lanczos_hbd_ladderILi")
    assert seen == len(STRIPS), seen
    assert not bad, bad[:5]
