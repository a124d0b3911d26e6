"""What the compiled unit of chv_scale_lanczos_from_yuv (swiftvideo_amd/csrc/kernels_lanczos_from_yuv.hip.cpp, DESIGN.md sections 4.4.6, 5 and
6) must look like, from the code object's metadata and disassembly only: exactly the five kernels DESIGN names and none of the other units',
no FLAT accesses, no scratch and no spill of either kind, the four strip variants inside the register budget of their stated occupancy (four
waves per SIMD), their hand-awaited loads untouched while in flight.  Reads the objects the build leaves in-tree (skipped when they are not
there); no GPU needed."""
import re
import subprocess
import sys
from pathlib import Path

from test_device_code_contract import LLVM, _code_object, _kernels

UNIT = "kernels_lanczos_from_yuv"
STRIP = "_ZN3chv22lanczos_from_yuv_stripILi{}ELi{}EEEvNS_11FromYuvArgsE"
TILE = "_ZN3chv21lanczos_from_yuv_tileENS_11FromYuvArgsE"
WAVES, VGPR_LIMIT = 4, 128          # every strip variant at four waves per SIMD, 512 / 4 registers
STRIPS = [STRIP.format(t, sc) for t in (12, 22) for sc in (1, 2)]
DESIGN_NAMES = ("lanczos_from_yuv_strip<12, 1>", "lanczos_from_yuv_strip<12, 2>", "lanczos_from_yuv_strip<22, 1>", "lanczos_from_yuv_strip<22, 2>",
                "lanczos_from_yuv_tile")


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
    assert f"{WAVES} waves per SIMD" in section6[section6.index("lanczos_from_yuv_strip<12, 1>"):][:4000]


def test_the_other_units_keep_their_kernels(tmp_path):
    """the new unit includes the planar and the 4:2:0 row code: those units' kernels are not instantiated in it, and theirs are untouched"""
    assert not any("planar_lanczos" in n or "lanczos_420" in n or "lanczos_yuv" in n or "lanczos3_" in n for n in _kernels(_code_object(tmp_path, UNIT)))
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_planar_ladder"))) == 3
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_planar"))) == 6
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_420"))) == 5
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_to_yuv"))) == TO_YUV_KERNELS


TO_YUV_KERNELS = 10         # lanczos_yuv_strip<6 .. 22> in steps of two, and lanczos_yuv_tile


def test_no_flat_accesses(tmp_path):
    asm = _asm(tmp_path)
    flat = [l.strip() for l in asm.splitlines() if re.search(r"\bflat_(load|store|atomic)", l)]
    assert not flat, f"FLAT accesses (use gld/gst/cld, pixel_math.hip.h): {flat[:3]}"
    assert re.search(r"\bglobal_(load|store)", asm), "no global accesses found: disassembly did not work"


def test_no_scratch_no_spill_and_the_stated_occupancy(tmp_path):
    k = _kernels(_code_object(tmp_path, UNIT))
    for name, m in k.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    for name in STRIPS:
        assert k[name]["vgpr_count"] <= VGPR_LIMIT, f"{name}: {k[name]['vgpr_count']} VGPRs, {WAVES} waves per SIMD allow {VGPR_LIMIT}"
    asm = _asm(tmp_path)
    assert not re.search(r"\b(scratch_(load|store)|buffer_(load|store)|v_writelane|v_readlane)", asm)


def test_hand_awaited_loads_are_not_touched_while_in_flight(tmp_path):
    """the strip bodies issue their row loads from inline asm and wait for them with a hand-written s_waitcnt: tools/check_inflight.py walks
    all four variants"""
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import check_inflight
    seen, bad = check_inflight.check(_asm(tmp_path), r"lanczos_from_yuv_stripILi")
    assert seen == len(STRIPS), seen
    assert not bad, bad[:5]
