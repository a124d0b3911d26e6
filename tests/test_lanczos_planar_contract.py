"""What the compiled planar Lanczos unit (swiftvideo_amd/csrc/kernels_lanczos_planar.hip.cpp, DESIGN.md sections 4.4 and 5) must look like: no
FLAT accesses, the wave-per-strip kernels without scratch and without spills inside the register budgets of the occupancy DESIGN.md section 6
states (five waves per SIMD up to 12 taps, four beyond) — and
the 4-component unit beside it holds exactly the kernels it held before the planar unit existed.  Reads the objects the build leaves in-tree
(skipped when they are not there); no GPU needed."""
import re
import subprocess
import sys
from pathlib import Path

from test_device_code_contract import LLVM, _code_object, _kernels

STRIP_TAPS = (6, 8, 12, 16, 22)

# kernels_lanczos.hip.o: the tile kernel's eleven instantiations, lanczos3_strip<6 .. 22>, lanczos3_strip2<even | odd>
BGRA_UNIT = sorted(
    [f"_ZN3chv13lanczos3_bgraILi{t}ELb{e}ELb{p}ELi{w}ELi{h}EEEvNS_6DPlaneES1_PKiPKfiS3_S5_iiiiPKS1_" for t, e, p, w, h in
     ((0, 0, 0, 32, 16), (0, 0, 0, 8, 4), (12, 0, 0, 32, 16), (12, 0, 1, 32, 16), (12, 1, 0, 32, 16), (12, 1, 1, 32, 16), (24, 0, 0, 32, 16),
      (24, 0, 0, 8, 4), (24, 0, 1, 32, 16), (6, 1, 0, 32, 16), (6, 1, 1, 32, 16))] +
    [f"_ZN3chv14lanczos3_stripILi{t}EEEvNS_6DPlaneES1_PKiPKfS3_S5_iiiiiPKS1_" for t in range(6, 23, 2)] +
    [f"_ZN3chv15lanczos3_strip2ILb{o}EEEvNS_6DPlaneES1_PKiPKfS3_S5_iiiiPKS1_" for o in (0, 1)])


def test_no_flat_accesses(tmp_path):
    co = _code_object(tmp_path, "kernels_lanczos_planar")
    asm = subprocess.run([LLVM / "llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    flat = [l.strip() for l in asm.splitlines() if re.search(r"\bflat_(load|store|atomic)", l)]
    assert not flat, f"FLAT accesses (use gld/gst/cld, pixel_math.hip.h): {flat[:3]}"
    assert re.search(r"\bglobal_(load|store)", asm), "no global accesses found: disassembly did not work"


def test_the_unit_holds_the_strip_kernels_and_the_tile_kernel(tmp_path):
    k = _kernels(_code_object(tmp_path, "kernels_lanczos_planar"))
    assert sorted(k) == sorted([f"_ZN3chv20planar_lanczos_stripILi{t}EEEvNS_10PlanarArgsE" for t in STRIP_TAPS] + ["_ZN3chv19planar_lanczos_tileENS_10PlanarArgsE"]), sorted(k)
    assert not any("lanczos3_strip" in n or "lanczos3_bgra" in n for n in k)


# waves per SIMD that DESIGN.md section 6 states for planar_lanczos_strip<T>, and the VGPR count that occupancy allows on gfx950 (512 per lane and SIMD)
STRIP_WAVES = {6: 5, 8: 5, 12: 5, 16: 4, 22: 4}
VGPR_LIMIT = {5: 96, 4: 128}


def test_strip_kernels_keep_their_stated_occupancy_without_scratch(tmp_path):
    """planar_lanczos_strip<T>: the window of T floats, the T horizontal weights and the prefetched vectors per lane fit the registers of the
    occupancy DESIGN.md section 6 states — five waves per SIMD up to 12 taps (at most 96 VGPRs), four beyond (at most 128) — with nothing
    spilled and no private segment"""
    k = _kernels(_code_object(tmp_path, "kernels_lanczos_planar"))
    strips = {n: m for n, m in k.items() if "planar_lanczos_strip" in n}
    assert len(strips) == len(STRIP_TAPS)
    for name, m in strips.items():
        taps = int(re.search(r"ILi(\d+)E", name).group(1))
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_LIMIT[STRIP_WAVES[taps]], (name, m)


def test_strip_kernels_store_dwords_and_stage_vectors(tmp_path):
    """the interior store of a strip is a dword per quad gathered with two quad-permute DPP moves, the staged rows arrive as 16-byte vectors"""
    co = _code_object(tmp_path, "kernels_lanczos_planar")
    asm = subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    bodies = re.split(r"\n[0-9a-f]+ <(_ZN3chv20planar_lanczos_strip[^>]*)>:\n", asm)
    assert len(bodies) == 1 + 2 * len(STRIP_TAPS)
    for name, body in zip(bodies[1::2], bodies[2::2]):
        assert "global_store_dword " in body and "quad_perm:[1,0,3,2]" in body and "quad_perm:[2,3,0,1]" in body, name
        assert "global_load_dwordx4" in body and "ds_write_b128" in body, name
        assert "scratch_" not in body, name


def test_the_bgra_unit_holds_exactly_the_kernels_it_held(tmp_path):
    assert sorted(_kernels(_code_object(tmp_path, "kernels_lanczos"))) == BGRA_UNIT


def test_hand_awaited_loads_are_not_touched_while_in_flight(tmp_path):
    """the interior strips of planar_lanczos_strip<T> issue their row loads from inline asm and wait for them with a hand-written s_waitcnt:
    the compiler does not know the destination registers are still being written.  tools/check_inflight.py walks every instantiation."""
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import check_inflight
    co = _code_object(tmp_path, "kernels_lanczos_planar")
    asm = subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    seen, bad = check_inflight.check(asm, "planar_lanczos_strip")
    assert seen == len(STRIP_TAPS), seen
    assert not bad, bad[:5]
    # the hand-written waits are there: PRE - 1 younger loads stay in flight (PRE = 4, 3 or 2 by tap count)
    bodies = re.split(r"\n[0-9a-f]+ <(_ZN3chv20planar_lanczos_strip[^>]*)>:\n", asm)
    for name, body in zip(bodies[1::2], bodies[2::2]):
        depth = {"Li6E": 3, "Li8E": 4, "Li12E": 4, "Li16E": 4, "Li22E": 2}[re.search(r"ILi\d+E", name).group(0)[1:]]
        assert f"s_waitcnt vmcnt({depth - 1})" in body, (name, depth)
