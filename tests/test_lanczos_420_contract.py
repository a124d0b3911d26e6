"""What the compiled unit of the 4:2:0 conversion entries (swiftvideo_amd/csrc/kernels_lanczos_420.hip.cpp, DESIGN.md sections 4.4.5, 5 and 6)
must look like, from the code object's metadata and disassembly only: exactly the five kernels DESIGN names and none of the other units', no
FLAT accesses, no scratch and no spill of either kind, the four strip variants inside the register budgets of their stated occupancy (five
waves per SIMD with the bodies up to 12 taps, four with all five), their hand-awaited loads untouched while in flight.  Reads the objects the
build leaves in-tree (skipped when they are not there); no GPU needed."""
import re
import subprocess
import sys
from pathlib import Path

from test_device_code_contract import LLVM, _code_object, _kernels

UNIT = "kernels_lanczos_420"
LADDER = "_ZN3chv18lanczos_420_ladderILi{}ELb{}EEEvNS_8X420ArgsE"
TILE = "_ZN3chv23lanczos_420_ladder_tileENS_8X420ArgsE"
# largest tap class a variant holds -> (waves per SIMD DESIGN.md section 6 states, the VGPR count that occupancy allows on gfx950, its bodies' tap classes)
VARIANTS = {12: (5, 96, (6, 8, 12)), 22: (4, 128, (6, 8, 12, 16, 22))}
STRIPS = [LADDER.format(t, d) for t in VARIANTS for d in (0, 1)]


def _asm(tmp_path):
    co = _code_object(tmp_path, UNIT)
    return subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout


def _bodies(asm):
    parts = re.split(r"\n[0-9a-f]+ <(_ZN3chv[^>]*)>:\n", asm)
    return dict(zip(parts[1::2], parts[2::2]))


def test_the_unit_holds_its_kernels_and_no_others(tmp_path):
    k = _kernels(_code_object(tmp_path, UNIT))
    assert sorted(k) == sorted(STRIPS + [TILE]), sorted(k)
    design = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    for name in ("lanczos_420_ladder<12, true>", "lanczos_420_ladder<12, false>", "lanczos_420_ladder<22, true>", "lanczos_420_ladder<22, false>",
                 "lanczos_420_ladder_tile"):
        assert name in design, name


def test_the_same_format_units_keep_their_kernels(tmp_path):
    """the new unit includes the planar row code for its luma planes: the planar units' kernels are not instantiated in it, and theirs are untouched"""
    assert not any("planar_lanczos" in n or "lanczos_yuv" in n or "lanczos3_" in n for n in _kernels(_code_object(tmp_path, UNIT)))
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_planar_ladder"))) == 3
    assert len(_kernels(_code_object(tmp_path, "kernels_lanczos_planar"))) == 6


def test_no_flat_accesses(tmp_path):
    asm = _asm(tmp_path)
    flat = [l.strip() for l in asm.splitlines() if re.search(r"\bflat_(load|store|atomic)", l)]
    assert not flat, f"FLAT accesses (use gld/gst/cld, pixel_math.hip.h): {flat[:3]}"
    assert re.search(r"\bglobal_(load|store)", asm), "no global accesses found: disassembly did not work"


def test_no_scratch_no_spill_and_the_stated_occupancy(tmp_path):
    k = _kernels(_code_object(tmp_path, UNIT))
    for name, m in k.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    for maxt, (waves, limit, _) in VARIANTS.items():
        for d in (0, 1):
            m = k[LADDER.format(maxt, d)]
            assert m["vgpr_count"] <= limit, f"lanczos_420_ladder<{maxt}, {bool(d)}>: {m['vgpr_count']} VGPRs, {waves} waves per SIMD allow {limit}"
    asm = _asm(tmp_path)
    assert not re.search(r"\b(scratch_(load|store)|buffer_(load|store)|v_writelane|v_readlane)", asm)


def test_every_body_is_in_its_variant(tmp_path):
    """a variant holds, per tap class it serves, the shared luma body and the chroma body of its direction: each tap class waits for its
    prefetched rows with its own depth (4, 3 or 2), stores dwords gathered with two quad-permute DPP moves and stages 16-byte vectors; the
    records and the planes come through the scalar unit"""
    bodies = _bodies(_asm(tmp_path))
    for maxt, (_, _, taps) in VARIANTS.items():
        for d in (0, 1):
            body = bodies[LADDER.format(maxt, d)]
            for depth in {4 if t % 4 == 0 else 3 if t % 3 == 0 else 2 for t in taps}:
                assert f"s_waitcnt vmcnt({depth - 1})" in body, (maxt, d, depth)
            # one epilogue per FAST body (luma and chroma): the drain of the rows requested past the strip's last one
            assert len(re.findall(r"s_waitcnt vmcnt\(0\)\s", body)) >= 2 * len(taps), (maxt, d)
            assert "global_store_dword " in body and "quad_perm:[1,0,3,2]" in body and "quad_perm:[2,3,0,1]" in body and "ds_write_b128" in body, (maxt, d)
            assert "ds_bpermute" not in body and "ds_swizzle" not in body, (maxt, d)
            assert re.search(r"s_load_dwordx[248]", body), (maxt, d)
    assert re.search(r"s_load_dwordx[248]", bodies[TILE])


def test_hand_awaited_loads_are_not_touched_while_in_flight(tmp_path):
    """the strip bodies issue their row loads from inline asm and wait for them with a hand-written s_waitcnt: tools/check_inflight.py walks
    all four variants"""
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import check_inflight
    seen, bad = check_inflight.check(_asm(tmp_path), r"lanczos_420_ladderILi")
    assert seen == len(STRIPS), seen
    assert not bad, bad[:5]
