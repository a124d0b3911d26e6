"""The chroma-carry kernels of tick_bgra_stream on the built gfx950 object (kernels_stream_carry.hip.o): three kernels, the register budget
of five waves per SIMD, the M0 and in-flight contracts of the family, and a row loop that exists in two copies ("the top chroma tap row
is the even set" / "the odd set") each of which is no longer than the row of its sibling in kernels_stream_opq.hip.o built from the same
tree — a register copy where the two copies join, or a select per carried byte, would show there.  Skipped where the objects are not
built; no GPU needed."""
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

NEW, SIB = CSRC / "kernels_stream_carry.hip.o", CSRC / "kernels_stream_opq.hip.o"


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    if not NEW.exists() or not SIB.exists() or not (row_loop_count.LLVM / "llvm-objcopy").exists():
        pytest.skip("the stream objects are not built here")
    return {o: row_loop_count.code_object(o, tmp_path_factory.mktemp(o.stem.replace(".", "_"))) for o in (NEW, SIB)}


@pytest.fixture(scope="module")
def new_kernels(objects):
    ks = row_loop_count.kernels(objects[NEW], prefix="_ZN3chv")
    return {n: i for n, i in ks.items() if "tick_bgra_stream" in n}


def test_names_and_instantiations(objects, new_kernels):
    """2, 3 and 4 layers, batch kernels only; `tick_bgra_stream` stays a prefix of the name (bench.py finds the headline's kernel in a
    profile by it)"""
    every = subprocess.run([row_loop_count.LLVM / "llvm-readelf", "--notes", objects[NEW]], check=True, capture_output=True, text=True).stdout
    assert len(re.findall(r"\.name:\s+_Z\S+", every)) == 3, "a kernel of another family in this unit"
    assert len(new_kernels) == 3, sorted(new_kernels)
    for nl in (2, 3, 4):
        assert sum(1 for n in new_kernels if n.startswith(f"_ZN3chv19tick_bgra_stream_ccILi{nl}EEE")) == 1


def test_registers_no_spill_no_scratch(objects, new_kernels):
    notes = subprocess.run([row_loop_count.LLVM / "llvm-readelf", "--notes", objects[NEW]], check=True, capture_output=True, text=True).stdout
    meta, cur = {}, None
    for line in notes.splitlines():
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
        assert m.get("group_segment_fixed_size", 0) == 0, (name, m)    # LDS is the launch's, sized as for the sibling
    assert seen == 3


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
    """lengths of the runs of consecutive ds_read_u8 (a hand-issued group is one asm statement)"""
    runs, n = [], 0
    for _, op, _ in loop:
        if op == "ds_read_u8":
            n += 1
        elif n:
            runs.append(n)
            n = 0
    return runs + ([n] if n else [])


@pytest.mark.parametrize("nl", [2, 3, 4])
def test_every_copy_of_the_row_is_no_longer_than_the_sibling(objects, new_kernels, nl):
    """Both copies keep the 15 v_fma_mix_f32 per layer and the one wait per layer, have no more vector instructions than
    tick_bgra_stream_ob's row (the two address adds of a parity's read stand where the four of the transient taps stood), and hold one
    group of 4 x NL chroma byte reads per parity — on the GPU a row issues one of them on three rows in four at 1.5 : 1 and none on the
    fourth — beside the 4 luma byte reads per layer."""
    old = row_loop_count.kernels(objects[SIB], prefix="_ZN3chv")
    sib = [i for n, i in old.items() if n.startswith(f"_ZN3chv19tick_bgra_stream_obILi{nl}ELb0ELb1E")]
    assert len(sib) == 1
    sib_loop = row_loop_count.row_loop(sib[0])
    sibling = row_loop_count.classes(sib_loop)
    assert sum(1 for _, op, _ in sib_loop if op == "v_fma_mix_f32") == 15 * nl
    hit = [i for n, i in new_kernels.items() if n.startswith(f"_ZN3chv19tick_bgra_stream_ccILi{nl}EEE")]
    assert len(hit) == 1
    copies = row_loop_count.row_loop_copies(hit[0])
    assert len(copies) == 2
    whole = row_loop_count.row_loop(hit[0])
    assert len(copies[0]) < len(whole) and len(copies[1]) < len(whole)
    for loop in copies:
        c = row_loop_count.classes(loop)
        print("sibling", sibling, "this copy", c)
        ops = [op for _, op, _ in loop]
        assert ops.count("v_fma_mix_f32") == 15 * nl
        assert c["valu"] <= sibling["valu"], (sibling, c)
        assert c["lgkm_waits"] <= sibling["lgkm_waits"] + 1, (sibling, c)
        runs = sorted(_byte_read_runs(loop))
        assert runs == [4] * nl + [4 * nl] * 2, runs              # luma per layer; one chroma group per parity, 4 x NL bytes each
        assert c["lds"] <= sibling["lds"], (sibling, c)           # statically both parities; dynamically at most one on most rows
