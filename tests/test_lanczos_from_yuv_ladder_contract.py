"""What the compiled unit of chv_scale_lanczos_from_yuv_ladder (swiftvideo_amd/csrc/kernels_lanczos_from_yuv_ladder.hip.cpp, DESIGN.md sections
4.4.7, 5 and 6) must look like, from the code object's metadata and disassembly only: exactly the five kernels DESIGN names and none of the
other units', no FLAT accesses, no scratch and no spill of either kind, the four strip variants inside the register budget of their stated
occupancy — four waves per SIMD, <22, .> included: it sits at 128 VGPRs, the last register of that budget, without a spill —, their
hand-awaited loads untouched while in flight.  Reads the objects the build leaves in-tree (skipped when they are not there); no GPU needed."""
import re
import subprocess
import sys
from pathlib import Path

from test_device_code_contract import LLVM, _code_object, _kernels

UNIT = "kernels_lanczos_from_yuv_ladder"
STRIP = "_ZN3chv23lanczos_from_yuv_ladderILi{}ELi{}EEEvNS_7FylArgsE"
TILE = "_ZN3chv28lanczos_from_yuv_ladder_tileENS_7FylArgsE"
WAVES, VGPR_LIMIT = 4, 128          # every strip variant at four waves per SIMD, 512 / 4 registers
STRIPS = [STRIP.format(t, sc) for t in (12, 22) for sc in (1, 2)]
DESIGN_NAMES = ("lanczos_from_yuv_ladder<12, 1>", "lanczos_from_yuv_ladder<12, 2>", "lanczos_from_yuv_ladder<22, 1>", "lanczos_from_yuv_ladder<22, 2>",
                "lanczos_from_yuv_ladder_tile")


def _asm(tmp_path):
    co = _code_object(tmp_path, UNIT)
    return subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout


def test_the_unit_holds_its_kernels_and_no_others(tmp_path):
    k = _kernels(_code_object(tmp_path, UNIT))
    assert sorted(k) == sorted(STRIPS + [TILE]), sorted(k)
    design = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    section6 = design[design.index("\n## 6"):]
    for name in DESIGN_NAMES:
        assert name in section6, name
    assert f"{WAVES} waves per SIMD" in section6[section6.index("lanczos_from_yuv_ladder<12, 1>"):][:4000]


def test_the_other_units_keep_their_kernels(tmp_path):
    """the new unit includes the single call's row code: that unit's kernels are not instantiated in it, and every other unit keeps its count"""
    assert not any("lanczos_from_yuv_strip" in n or "lanczos_from_yuv_tile" in n or "planar_lanczos" in n or "lanczos_420" in n or "lanczos_yuv" in n
                   or "lanczos3_" in n for n in _kernels(_code_object(tmp_path, UNIT)))
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_from_yuv"))) == 5
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_planar_ladder"))) == 3
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_planar"))) == 6
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_420"))) == 5
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_to_yuv"))) == 10      # lanczos_yuv_strip<6 .. 22> in steps of two, and lanczos_yuv_tile


def test_no_flat_accesses(tmp_path):
    asm = _asm(tmp_path)
    flat = [l.strip() for l in asm.splitlines() if re.search(r"\bflat_(load|store|atomic)", l)]
    assert not flat, f"FLAT accesses (use gld/gst/cld, pixel_math.hip.h): {flat[:3]}"
    assert re.search(r"\bglobal_(load|store)", asm), "no global accesses found: disassembly did not work"


def test_no_scratch_no_spill_and_the_stated_occupancy(tmp_path):
    k = _kernels(_code_object(tmp_path, UNIT))
    assert len(k) == 5
    for name, m in k.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    for name in STRIPS:
        assert k[name]["vgpr_count"] <= VGPR_LIMIT, f"{name}: {k[name]['vgpr_count']} VGPRs, {WAVES} waves per SIMD allow {VGPR_LIMIT}"


def test_hand_awaited_loads_are_not_touched_while_in_flight(tmp_path):
    """the strip bodies issue their row loads from inline asm and wait for them with a hand-written s_waitcnt: tools/check_inflight.py walks
    all four variants"""
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import check_inflight
    seen, bad = check_inflight.check(_asm(tmp_path), r"lanczos_from_yuv_ladderILi")
    assert seen == len(STRIPS), seen
    assert not bad, bad[:5]
