"""What the compiled unit of chv_scale_lanczos_rgb_ladder (swiftvideo_amd/csrc/kernels_lanczos_rgb_ladder.hip.cpp, DESIGN.md sections 4.4.8, 5
and 6) must look like, from the code object's metadata and disassembly only: exactly the three kernels DESIGN names and none of the other
units', no FLAT accesses, no scratch and no spill of either kind, the two strip bodies inside the register budget of their stated occupancy
— <12> at four waves per SIMD (128 VGPRs), <22> at three (168) —, their hand-awaited loads untouched while in flight.  Reads the objects the
build leaves in-tree (skipped when they are not there); no GPU needed."""
import re
import subprocess
import sys
from pathlib import Path

from test_device_code_contract import LLVM, _code_object, _kernels

UNIT = "kernels_lanczos_rgb_ladder"
STRIP = "_ZN3chv18lanczos_rgb_ladderILi{}EEEvNS_13RgbLadderArgsE"
TILE = "_ZN3chv23lanczos_rgb_ladder_tileENS_13RgbLadderArgsE"
# waves per SIMD and the registers floor(512 / waves) leaves, in allocation granules of 8
BUDGET = {12: (4, 128), 22: (3, 168)}
DESIGN_NAMES = ("lanczos_rgb_ladder<12>", "lanczos_rgb_ladder<22>", "lanczos_rgb_ladder_tile")


def _asm(tmp_path):
    co = _code_object(tmp_path, UNIT)
    return subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout


def test_the_unit_holds_its_kernels_and_no_others(tmp_path):
    k = _kernels(_code_object(tmp_path, UNIT))
    assert sorted(k) == sorted([STRIP.format(12), STRIP.format(22), TILE]), sorted(k)
    assert not any("lanczos3_" in n or "planar_lanczos" in n or "lanczos_420" in n or "lanczos_yuv" in n or "lanczos_from_yuv" in n for n in k)
    design = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    section6 = design[design.index("\n## 6"):]
    for name in DESIGN_NAMES:
        assert name in section6, name
    ours = " ".join(section6[section6.index("lanczos_rgb_ladder<12>"):][:4000].split())          # (the paragraph, line breaks aside)
    assert "four waves per SIMD" in ours and "three waves per SIMD" in ours
    for waves, limit in BUDGET.values():
        assert limit == 512 // waves // 8 * 8


def test_the_other_units_keep_their_kernels(tmp_path):
    assert len([n for n in _kernels(_code_object(tmp_path, "kernels_lanczos")) if "lanczos3_strip" in n]) == 11
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_from_yuv_ladder"))) == 5
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_from_yuv"))) == 5
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_planar_ladder"))) == 3
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_planar"))) == 6
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_420"))) == 5
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_to_yuv"))) == 10


def test_no_flat_accesses(tmp_path):
    asm = _asm(tmp_path)
    flat = [l.strip() for l in asm.splitlines() if re.search(r"\bflat_(load|store|atomic)", l)]
    assert not flat, f"FLAT accesses (use gld/gst/cld, pixel_math.hip.h): {flat[:3]}"
    assert re.search(r"\bglobal_(load|store)", asm), "no global accesses found: disassembly did not work"


def test_no_scratch_no_spill_and_the_stated_occupancy(tmp_path):
    k = _kernels(_code_object(tmp_path, UNIT))
    assert len(k) == 3
    for name, m in k.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    for t, (waves, limit) in BUDGET.items():
        got = k[STRIP.format(t)]["vgpr_count"]
        assert got <= limit, f"<{t}>: {got} VGPRs, {waves} waves per SIMD allow {limit}"


def test_hand_awaited_loads_are_not_touched_while_in_flight(tmp_path):
    """the strip bodies issue their row loads from inline asm and wait for them with a hand-written s_waitcnt: tools/check_inflight.py walks both"""
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import check_inflight
    seen, bad = check_inflight.check(_asm(tmp_path), r"lanczos_rgb_ladderILi")
    assert seen == 2, seen
    assert not bad, bad[:5]
