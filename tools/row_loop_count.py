#!/usr/bin/env python3
"""tools/row_loop_count.py <object.o> [name fragment] — instruction classes inside the ROW LOOP of the tick_bgra_stream kernels of a built
object: the widest backward branch whose range holds every v_fma_mix_f32 of the kernel (the loop over canvas rows is the kernel's
outermost loop; the request loops and the table refill lie inside it).  Static counts over the whole range, every path together: what tests/test_stream_row_control_contract.py bounds."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")


def code_object(obj, tmp):
    fat, co = Path(tmp) / "k.fatbin", Path(tmp) / "k.co"
    subprocess.run([LLVM / "llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", str(obj), str(Path(tmp) / "copy.o")], check=True)
    subprocess.run([LLVM / "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={co}"], check=True)
    return co


def kernels(co, prefix="_ZN3chv16tick_bgra_stream"):
    """{mangled name: [(address, mnemonic, operands)]}"""
    asm = subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", str(co)], check=True, capture_output=True, text=True).stdout
    parts = re.split(r"\n[0-9a-f]+ <(_Z[^>]*)>:\n", asm)
    out = {}
    for name, body in zip(parts[1::2], parts[2::2]):
        if not name.startswith(prefix):
            continue
        ins = []
        for line in body.splitlines():
            m = re.match(r"\s*(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
            if m:
                t = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>\s*$", line)
                ins.append((int(m.group(3), 16), m.group(1), m.group(2) + (" " + t.group(0).strip() if t else "")))
        out[name] = ins
    return out


def row_loop(ins):
    """the instructions of the outermost loop that holds every v_fma_mix_f32"""
    mix = [a for a, op, _ in ins if op == "v_fma_mix_f32"]
    if not mix:
        return []
    best = None
    for a, op, args in ins:
        if not op.startswith("s_cbranch") and op != "s_branch":
            continue
        m = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", args)
        if not m:
            continue
        tgt = ins[0][0] + int(m.group(1), 16)       # (targets print as <kernel+0xoffset>)
        if tgt <= min(mix) and a >= max(mix) and (best is None or a - tgt > best[1] - best[0]):
            best = (tgt, a)
    if best is None:
        return []
    return [i for i in ins if best[0] <= i[0] <= best[1]]


def classes(loop):
    c = {"total": len(loop), "lgkm_waits": 0, "vm_waits": 0, "salu": 0, "branches": 0, "valu": 0, "lds": 0, "readfirstlane": 0}
    for _, op, args in loop:
        if op == "s_waitcnt":
            if "lgkmcnt" in args:
                c["lgkm_waits"] += 1
            if "vmcnt" in args:
                c["vm_waits"] += 1
        elif op.startswith("s_cbranch") or op == "s_branch":
            c["branches"] += 1
        elif op in ("s_nop", "s_endpgm", "s_barrier"):
            pass
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if op == "v_readfirstlane_b32":
                c["readfirstlane"] += 1
    return c


def count(obj, fragment=""):
    with tempfile.TemporaryDirectory() as tmp:
        ks = kernels(code_object(obj, tmp))
    return {n: classes(row_loop(i)) for n, i in ks.items() if fragment in n}


if __name__ == "__main__":
    for name, c in sorted(count(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "").items()):
        print(name[:60], " ".join(f"{k}={v}" for k, v in c.items()))
