"""What the compiled Lanczos-to-YUV unit (swiftvideo_amd/csrc/kernels_lanczos_to_yuv.hip.cpp, DESIGN.md sections 4.4.2 and 6) must look like: no
FLAT accesses, the wave-per-strip kernels without scratch and without spills inside the register budgets of the occupancy DESIGN.md section 6
states (four waves per SIMD up to 16 taps, three from 18 on), their hand-awaited loads untouched while in flight, and exactly the kernels DESIGN
names — the 4-component unit beside it holds exactly the kernels it held.  Reads the objects the build leaves in-tree (skipped when they are not
there); no GPU needed."""
import re
import subprocess
import sys
from pathlib import Path

from test_device_code_contract import LLVM, _code_object, _kernels
from test_lanczos_planar_contract import BGRA_UNIT

UNIT = "kernels_lanczos_to_yuv"
STRIP_TAPS = tuple(range(6, 23, 2))
STRIP = "_ZN3chv17lanczos_yuv_stripILi{}EEEvNS_9ToYuvArgsE"
TILE = "_ZN3chv16lanczos_yuv_tileENS_9ToYuvArgsE"


def _asm(tmp_path):
    co = _code_object(tmp_path, UNIT)
    return subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout


def _strip_bodies(asm):
    bodies = re.split(r"\n[0-9a-f]+ <(_ZN3chv17lanczos_yuv_strip[^>]*)>:\n", asm)
    assert len(bodies) == 1 + 2 * len(STRIP_TAPS)
    return list(zip(bodies[1::2], bodies[2::2]))


def test_no_flat_accesses(tmp_path):
    asm = _asm(tmp_path)
    flat = [l.strip() for l in asm.splitlines() if re.search(r"\bflat_(load|store|atomic)", l)]
    assert not flat, f"FLAT accesses (use gld/gst/cld, pixel_math.hip.h): {flat[:3]}"
    assert re.search(r"\bglobal_(load|store)", asm), "no global accesses found: disassembly did not work"


def test_the_unit_holds_the_strip_kernels_and_the_tile_kernel(tmp_path):
    k = _kernels(_code_object(tmp_path, UNIT))
    assert sorted(k) == sorted([STRIP.format(t) for t in STRIP_TAPS] + [TILE]), sorted(k)
    assert not any("lanczos3_" in n or "planar_lanczos" in n for n in k)


def test_the_bgra_unit_holds_exactly_the_kernels_it_held(tmp_path):
    assert sorted(_kernels(_code_object(tmp_path, "kernels_lanczos"))) == BGRA_UNIT


# waves per SIMD that DESIGN.md section 6 states for lanczos_yuv_strip<T>, and the VGPR count that occupancy allows on gfx950 (512 per lane and SIMD)
STRIP_WAVES = {6: 4, 8: 4, 10: 4, 12: 4, 14: 4, 16: 4, 18: 3, 20: 3, 22: 3}
VGPR_LIMIT = {4: 128, 3: 168}


def test_strip_kernels_keep_their_stated_occupancy_without_scratch(tmp_path):
    """lanczos_yuv_strip<T>: the window of 3 T floats, the T horizontal weights, the T staged texels and the prefetched vectors per lane fit the
    registers of the occupancy DESIGN.md section 6 states, with nothing spilled — vector or scalar — and no private segment"""
    k = _kernels(_code_object(tmp_path, UNIT))
    strips = {n: m for n, m in k.items() if "lanczos_yuv_strip" in n}
    assert len(strips) == len(STRIP_TAPS)
    for name, m in strips.items():
        taps = int(re.search(r"ILi(\d+)E", name).group(1))
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_LIMIT[STRIP_WAVES[taps]], (name, m)
    tile = k[TILE]
    assert tile["vgpr_spill_count"] == 0 and tile["sgpr_spill_count"] == 0 and tile["private_segment_fixed_size"] == 0, tile


def test_strip_kernels_store_dwords_and_stage_vectors(tmp_path):
    """the luma of a quad leaves as one dword gathered with two quad-permute DPP moves, the column pair's chroma sums cross through DPP (no LDS
    beyond the staging ring: one 128-bit write per staged row and lane), the staged rows arrive as 16-byte vectors"""
    for name, body in _strip_bodies(_asm(tmp_path)):
        assert "global_store_dword " in body and "quad_perm:[1,0,3,2]" in body and "quad_perm:[2,3,0,1]" in body, name
        assert "global_load_dwordx4" in body and "ds_write_b128" in body, name
        assert "scratch_" not in body and "ds_bpermute" not in body and "ds_swizzle" not in body, name
        assert not re.search(r"\bds_write_b(8|16|32|64)\b", body), name


def test_hand_awaited_loads_are_not_touched_while_in_flight(tmp_path):
    """lanczos_yuv_strip<T> issues its row loads from inline asm and waits for them with a hand-written s_waitcnt: the compiler does not know the
    destination registers are still being written.  tools/check_inflight.py walks every instantiation."""
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import check_inflight
    asm = _asm(tmp_path)
    seen, bad = check_inflight.check(asm, "lanczos_yuv_strip")
    assert seen == len(STRIP_TAPS), seen
    assert not bad, bad[:5]
    # the hand-written waits are there: PRE - 1 younger loads stay in flight (PRE = 4, 3 or 2 by tap count), and the row loop holds no other
    # vector load that would count among them
    for name, body in _strip_bodies(asm):
        taps = int(re.search(r"ILi(\d+)E", name).group(1))
        depth = 4 if taps % 4 == 0 else 3 if taps % 3 == 0 else 2
        assert f"s_waitcnt vmcnt({depth - 1})" in body, (name, depth)
