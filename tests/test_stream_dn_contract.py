"""The f32-tap kernels of tick_bgra_stream on the built gfx950 object (kernels_stream_dn.hip.o): three kernels, the register budget of five
waves per SIMD, the M0 and in-flight contracts of the family, an FP mode that keeps binary32 denormals (the taps ARE denormals), and a row
whose two copies each hold only the blend's 3 x NL v_fma_mix_f32 — the twelve taps per layer went to v_fma_f32 / v_fmac_f32 — with no
conversion instruction and no more vector instructions, LDS instructions and LDS waits than the corresponding copy of tick_bgra_stream_cc
(kernels_stream_carry.hip.o) built from the same tree, and the same byte-read groups.  Skipped where the objects are not built; no GPU
needed."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "swiftvideo_amd" / "csrc"
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import row_loop_count  # noqa: E402
from test_stream_row_control_contract import inflight_violations  # noqa: E402

NEW, SIB = CSRC / "kernels_stream_dn.hip.o", CSRC / "kernels_stream_carry.hip.o"


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    if not NEW.exists() or not SIB.exists() or not (row_loop_count.LLVM / "llvm-objcopy").exists():
        pytest.skip("the stream objects are not built here")
    return {o: row_loop_count.code_object(o, tmp_path_factory.mktemp(o.stem.replace(".", "_"))) for o in (NEW, SIB)}


@pytest.fixture(scope="module")
def new_kernels(objects):
    ks = row_loop_count.kernels(objects[NEW], prefix="_ZN3chv")
    return {n: i for n, i in ks.items() if "tick_bgra_stream" in n}


def _notes(co):
    return subprocess.run([row_loop_count.LLVM / "llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout


def test_names_and_instantiations(objects, new_kernels):
    """2, 3 and 4 layers; `tick_bgra_stream` stays a prefix of the name (bench.py finds the headline's kernel in a profile by it)"""
    assert len(re.findall(r"\.name:\s+_Z\S+", _notes(objects[NEW]))) == 3, "a kernel of another family in this unit"
    assert len(new_kernels) == 3, sorted(new_kernels)
    for nl in (2, 3, 4):
        assert sum(1 for n in new_kernels if n.startswith(f"_ZN3chv19tick_bgra_stream_cdILi{nl}EEE")) == 1


def test_registers_no_spill_no_scratch(objects):
    meta, cur = {}, None
    for line in _notes(objects[NEW]).splitlines():
        m = re.match(r"\s*\.(name|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            cur = meta.setdefault(m.group(2), {})
        elif m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    seen = 0
    for name, m in meta.items():
        if "tick_bgra_stream" not in name:
            continue
        seen += 1
        print(name[:40], m)
        assert m["vgpr_count"] <= 96, (name, m)                        # five waves per SIMD
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m.get("private_segment_fixed_size", 0) == 0, (name, m)
        assert m.get("group_segment_fixed_size", 0) == 0, (name, m)
    assert seen == 3


def test_the_fp_mode_keeps_binary32_denormals(objects, tmp_path):
    """FLOAT_DENORM_MODE_32 is bits 16-17 of compute_pgm_rsrc1, the dword at offset 48 of a kernel descriptor (the `.kd` symbol): 3 = denormals
    are operands and results (what the assembler writes as .amdhsa_float_denorm_mode_32 3); the binary16 / binary64 field beside it (bits
    18-19, what the blend's code_h relies on) stays 3 too"""
    syms = subprocess.run([row_loop_count.LLVM / "llvm-readelf", "-s", "-S", "-W", objects[NEW]], check=True, capture_output=True, text=True).stdout
    sec = re.search(r"\]\s+\.rodata\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", syms)
    assert sec, "no .rodata"
    addr, off = int(sec.group(1), 16), int(sec.group(2), 16)
    blob = Path(objects[NEW]).read_bytes()
    kds = set(re.findall(r"^\s*\d+:\s+([0-9a-f]+)\s+64\s+OBJECT\s+\S+\s+\S+\s+\d+\s+(\S*tick_bgra_stream_cd\S*\.kd)\s*$", syms, re.M))       # (.dynsym and .symtab both list them)
    assert len(kds) == 3, kds
    for value, name in kds:
        at = int(value, 16) - addr + off
        rsrc1 = int.from_bytes(blob[at + 48:at + 52], "little")
        assert (rsrc1 >> 16) & 3 == 3 and (rsrc1 >> 18) & 3 == 3, (name, hex(rsrc1))


def test_m0_flat_and_hand_issued_reads_in_flight(objects, new_kernels):
    asm = subprocess.run([row_loop_count.LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", objects[NEW]], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"\bflat_(load|store|atomic)", asm)
    lines = [l.split("//")[0].strip() for l in asm.splitlines()]
    lines = [l for l in lines if l and not l.endswith(":")]
    dma = [i for i, l in enumerate(lines) if l.startswith("global_load_lds_dwordx4")]
    assert len(dma) >= 6
    for i in dma:
        assert any(l.startswith("s_mov_b32 m0") for l in lines[max(0, i - 3):i]), lines[max(0, i - 3):i + 1]
    others = [l for l in lines if re.search(r"\bm0\b", l) and not l.startswith("s_mov_b32 m0")]
    assert not others, others[:3]
    for name, ins in new_kernels.items():
        bad = inflight_violations(ins)
        assert not bad, (name, bad[:4])


def _byte_read_runs(loop):
    runs, n = [], 0
    for _, op, _ in loop:
        if op == "ds_read_u8":
            n += 1
        elif n:
            runs.append(n)
            n = 0
    return runs + ([n] if n else [])


@pytest.mark.parametrize("nl", [2, 3, 4])
def test_every_copy_of_the_row_against_the_carry_kernel(objects, new_kernels, nl):
    old = row_loop_count.kernels(objects[SIB], prefix="_ZN3chv")
    sib = [i for n, i in old.items() if n.startswith(f"_ZN3chv19tick_bgra_stream_ccILi{nl}EEE")]
    assert len(sib) == 1
    sib_copies = row_loop_count.row_loop_copies(sib[0])
    hit = [i for n, i in new_kernels.items() if n.startswith(f"_ZN3chv19tick_bgra_stream_cdILi{nl}EEE")]
    assert len(hit) == 1
    copies = row_loop_count.row_loop_copies(hit[0], min_mix=3 * nl)
    assert len(copies) == 2 and len(sib_copies) == 2
    whole = row_loop_count.row_loop(hit[0])
    assert len(copies[0]) < len(whole) and len(copies[1]) < len(whole)
    for loop, sib_loop in zip(copies, sib_copies):
        c, s = row_loop_count.classes(loop), row_loop_count.classes(sib_loop)
        print("carry copy", s, "this copy", c)
        ops = [op for _, op, _ in loop]
        assert ops.count("v_fma_mix_f32") == 3 * nl, ops.count("v_fma_mix_f32")
        assert [op for _, op, _ in sib_loop].count("v_fma_mix_f32") == 15 * nl
        assert not [op for op in ops if op.startswith("v_cvt_f32_ubyte")]
        assert c["valu"] <= s["valu"], (s, c)
        assert c["lds"] <= s["lds"], (s, c)
        assert c["lgkm_waits"] <= s["lgkm_waits"], (s, c)
        assert sorted(_byte_read_runs(loop)) == sorted(_byte_read_runs(sib_loop)) == [4] * nl + [4 * nl] * 2
