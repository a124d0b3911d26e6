"""What the compiled scatter kernels of chv_batch_rebind (swiftvideo_amd/csrc/kernels_rebind.hip.cpp) must look like, read from the gfx950 code
object inside the built library: no scratch segment, no LDS, a handful of registers, and exactly one memory write each — a 64-bit global
VECTOR store (one lane per {offset, address} pair).  No GPU needed."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")
KERNELS = ("batch_rebind_scatter", "batch_rebind_scatter_args")
STORE = "global_store_dwordx2"


@pytest.fixture(scope="module")
def code_object(built, tmp_path_factory):
    if not (LLVM / "llvm-objcopy").exists():
        pytest.skip("no LLVM binary tools here")
    tmp = tmp_path_factory.mktemp("rebind_co")
    fat, co = tmp / "lib.fatbin", tmp / "lib.co"
    subprocess.run([LLVM / "llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", built, tmp / "copy.so"], check=True)
    # the library's section holds one bundle per translation unit, back to back: the one that names the kernel
    blob, magic = fat.read_bytes(), b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    mine = [blob[a:b] for a, b in zip(starts, starts[1:] + [len(blob)]) if b"batch_rebind_scatter" in blob[a:b]]
    assert len(mine) == 1, f"{len(mine)} of {len(starts)} code bundles of {built.name} name the scatter kernel: is kernels_rebind.hip.cpp linked?"
    fat.write_bytes(mine[0])
    subprocess.run([LLVM / "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    return co


def _metadata(co):
    """{mangled name: {field: int}} from the code object's metadata note (one `  - .field:` block per kernel)"""
    notes = subprocess.run([LLVM / "llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n  - (?=\.)", notes)[1:]:
        name = re.search(r"^\s*\.name:\s+(_Z\S+)", block, re.M)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"^    \.([a-z_]+):\s+(\d+)\s*$", "    " + block, re.M)}
    return out


def _bodies(co):
    asm = subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    parts = re.split(r"\n[0-9a-f]+ <([^>]+)>:\n", asm)
    return {name: [l.split("//")[0].strip() for l in body.splitlines() if l.strip()] for name, body in zip(parts[1::2], parts[2::2])}


def _mangled(names, kernel):
    hits = [n for n in names if re.fullmatch(rf"_ZN3chv{len(kernel)}{kernel}E.*", n)]
    assert len(hits) == 1, (kernel, hits)
    return hits[0]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_lds_few_registers(code_object, kernel):
    meta = _metadata(code_object)
    m = meta[_mangled(meta, kernel)]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == 0, m
    assert m["vgpr_count"] <= 12, m
    # the list of the by-value twin is the launch's argument: block, count and 220 pairs inside the 4 KB kernarg segment
    assert m["kernarg_segment_size"] <= 4096 and (kernel != "batch_rebind_scatter_args" or m["kernarg_segment_size"] >= 16 + 220 * 16), m


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_only_memory_write_is_one_64_bit_global_vector_store(code_object, kernel):
    bodies = _bodies(code_object)
    body = bodies[_mangled(bodies, kernel)]
    assert any(l.startswith("s_endpgm") for l in body), "disassembly did not work"
    stores = [l for l in body if re.match(r"[a-z0-9_]*(store|atomic|_wb|discard)", l.split()[0])]
    assert len(stores) == 1 and stores[0].startswith(STORE + " "), stores
    # nothing else writes memory: every other memory instruction is a load, and none of them is a FLAT, scratch, buffer or LDS access
    memory = [l for l in body if re.match(r"(global|flat|scratch|buffer|ds)_", l.split()[0])]
    assert len(memory) >= 2, memory
    for l in memory:
        op = l.split()[0]
        assert op == STORE or op.startswith("global_load_"), l
