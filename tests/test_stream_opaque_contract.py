"""The opaque-bottom kernels of tick_bgra_stream on the built gfx950 object (kernels_stream_opq.hip.o): the register budget, the M0 and
in-flight contracts of the kernels they replace, and a row that is SHORTER than its sibling's in kernels_stream.hip.o built from the same
tree — vector instructions are what this kernel's time is made of (profiles/stream_opaque_bottom_notes.md).  Skipped where the objects are
not built; no GPU needed."""
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

NEW, OLD = CSRC / "kernels_stream_opq.hip.o", CSRC / "kernels_stream.hip.o"


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    if not NEW.exists() or not OLD.exists() or not (row_loop_count.LLVM / "llvm-objcopy").exists():
        pytest.skip("the stream objects are not built here")
    return {o: row_loop_count.code_object(o, tmp_path_factory.mktemp(o.stem.replace(".", "_"))) for o in (NEW, OLD)}


@pytest.fixture(scope="module")
def new_kernels(objects):
    ks = row_loop_count.kernels(objects[NEW], prefix="_ZN3chv")
    return {n: i for n, i in ks.items() if "tick_bgra_stream" in n}


def row_loops(ins):
    """every outermost loop of a kernel that holds a whole row (the v_fma_mix_f32 of all its layers): one per copy of the row loop"""
    mix = sum(1 for _, op, _ in ins if op == "v_fma_mix_f32")
    spans = []
    for a, op, args in ins:
        m = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", args) if (op.startswith("s_cbranch") or op == "s_branch") else None
        if m and ins[0][0] + int(m.group(1), 16) < a:
            spans.append((ins[0][0] + int(m.group(1), 16), a))
    outer = [s for s in spans if not any(o != s and o[0] <= s[0] and s[1] <= o[1] for o in spans)]
    loops = [[i for i in ins if lo <= i[0] <= hi] for lo, hi in sorted(outer)]
    loops = [l for l in loops if sum(1 for _, op, _ in l if op == "v_fma_mix_f32") >= 12]
    assert sum(sum(1 for _, op, _ in l if op == "v_fma_mix_f32") for l in loops) == mix, "a v_fma_mix_f32 outside the row loops"
    return loops


def test_names_and_instantiations(new_kernels):
    """2 - 4 layers x NV12 / planar, as the batch kernel and as its by-value twin; `tick_bgra_stream` stays a prefix of the name (bench.py
    finds the headline's kernel in a profile by it)"""
    assert len(new_kernels) == 12, sorted(new_kernels)
    for nl in (2, 3, 4):
        for pl in (0, 1):
            assert sum(1 for n in new_kernels if n.startswith(f"_ZN3chv19tick_bgra_stream_obILi{nl}ELb{pl}ELb1E")) == 1
            assert sum(1 for n in new_kernels if n.startswith(f"_ZN3chv23tick_bgra_stream_ob_oneILi{nl}ELb{pl}ELb1E")) == 1


def test_registers_no_spill_no_scratch(objects, new_kernels):
    notes = subprocess.run([row_loop_count.LLVM / "llvm-readelf", "--notes", objects[NEW]], check=True, capture_output=True, text=True).stdout
    meta, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*\.(name|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            cur = meta.setdefault(m.group(2), {})
        elif m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    seen = 0
    for name, m in meta.items():
        if "tick_bgra_stream" not in name:
            continue
        seen += 1
        assert m["vgpr_count"] <= 80, (name, m)                        # six waves per SIMD
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m.get("private_segment_fixed_size", 0) == 0, (name, m)
    assert seen == 12


def test_m0_flat_and_tap_reads_in_flight(objects, new_kernels):
    asm = subprocess.run([row_loop_count.LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", objects[NEW]], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"\bflat_(load|store|atomic)", asm)
    lines = [l.split("//")[0].strip() for l in asm.splitlines()]
    lines = [l for l in lines if l and not l.endswith(":")]
    dma = [i for i, l in enumerate(lines) if l.startswith("global_load_lds_dwordx4")]
    assert len(dma) >= 8
    for i in dma:
        assert any(l.startswith("s_mov_b32 m0") for l in lines[max(0, i - 3):i]), lines[max(0, i - 3):i + 1]
    others = [l for l in lines if re.search(r"\bm0\b", l) and not l.startswith("s_mov_b32 m0")]
    assert not others, others[:3]
    for name, ins in new_kernels.items():
        assert sum(1 for _, op, _ in ins if op == "ds_read_u8") >= 24, name
        bad = inflight_violations(ins)
        assert not bad, (name, bad[:4])


@pytest.mark.parametrize("pl", [0, 1], ids=["nv12", "y420p"])
@pytest.mark.parametrize("nl", [2, 3, 4])
def test_row_is_shorter_than_its_sibling(objects, new_kernels, nl, pl):
    """Every form against the kernel it replaces, built from the same tree: the row loop keeps its 15 v_fma_mix_f32 per layer (12 taps + 3
    blend inputs: the bottom layer's three moved into layer 1), the byte reads and the one wait per layer, has exactly 3 v_add_f32 and
    3 v_fma_f32 fewer (the bottom layer's rounding add, layer 1's inner term), and at least 5 vector instructions fewer in all (the six,
    less the compiler's freedom)."""
    inst = f"ILi{nl}ELb{pl}ELb1E"
    old = row_loop_count.kernels(objects[OLD], prefix="_ZN3chv")
    sib = [i for n, i in old.items() if n.startswith("_ZN3chv16tick_bgra_stream" + inst)]
    assert len(sib) == 1
    sib_loop = row_loop_count.row_loop(sib[0])
    sibling = row_loop_count.classes(sib_loop)
    sib_ops = [op for _, op, _ in sib_loop]
    hit = [i for n, i in new_kernels.items() if n.startswith("_ZN3chv19tick_bgra_stream_ob" + inst)]
    assert len(hit) == 1
    loops = row_loops(hit[0])
    assert len(loops) >= 1
    for loop in loops:
        c = row_loop_count.classes(loop)
        print("sibling", sibling, "this", c)
        ops = [op for _, op, _ in loop]
        assert ops.count("v_fma_mix_f32") == sib_ops.count("v_fma_mix_f32") == 15 * nl
        assert c["lds"] >= 12 * nl + 2 and c["lgkm_waits"] <= 10, c
        assert sibling["valu"] - c["valu"] >= 5, (sibling, c)
        assert sib_ops.count("v_add_f32_e32") - ops.count("v_add_f32_e32") == 3 and sib_ops.count("v_fma_f32") - ops.count("v_fma_f32") == 3
