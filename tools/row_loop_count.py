#!/usr/bin/env python3
"""tools/row_loop_count.py <object.o> [name fragment] — instruction classes inside the ROW LOOP of the tick_bgra_stream kernels of a built
object: the widest backward branch whose range holds every v_fma_mix_f32 of the kernel (the loop over canvas rows is the kernel's
outermost loop; the request loops and the table refill lie inside it).  Static counts over the whole range, every path together: what tests/test_stream_row_control_contract.py bounds.
A kernel whose row exists in two copies behind a uniform branch (kernels_stream_carry.hip.o) is reported per copy as well: row_loop_copies."""
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


def kernels(co, prefix="_ZN3chv1"):
    """{mangled name: [(address, mnemonic, operands)]}"""
    asm = subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", str(co)], check=True, capture_output=True, text=True).stdout
    parts = re.split(r"\n[0-9a-f]+ <(_Z[^>]*)>:\n", asm)
    out = {}
    for name, body in zip(parts[1::2], parts[2::2]):
        if not name.startswith(prefix) or "tick_bgra_stream" not in name:
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


def _target(ins, op, args):
    """address a branch instruction names, None for anything else"""
    if not op.startswith("s_cbranch") and op != "s_branch":
        return None
    m = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", args)
    return ins[0][0] + int(m.group(1), 16) if m else None


def row_loop_copies(ins, min_mix=12):
    """The row loop of a kernel whose row exists in more than one copy behind a uniform branch (the chroma-carry kernels: "the top tap row
    is the even set" / "the odd set"): a list with, per copy, the instructions a row that takes THAT copy passes through — the loop
    without the other copies.  A copy is the range a forward branch inside the loop jumps over, if that range holds the arithmetic of
    a row's layers (`min_mix` v_fma_mix_f32 or more: twelve by default; the f32-tap kernels of kernels_stream_dn.hip.o keep three per layer) and no
    smaller such range lies inside it: hipcc lays `if (p) A else B` out as "skip A
    unless p; A; skip B if p; B" or as "branch to B; A; jump over B; B", and both jump over each copy once.  A kernel with one copy
    gives a list of one: row_loop(ins)."""
    loop = row_loop(ins)
    if not loop:
        return []
    lo, hi = loop[0][0], loop[-1][0]
    mix = [a for a, op, _ in loop if op == "v_fma_mix_f32"]
    spans = []
    for a, op, args in loop:
        t = _target(ins, op, args)
        if t is not None and a < t <= hi + 4 and sum(1 for m in mix if a < m < t) >= min_mix:
            spans.append((a, t))
    spans = sorted(set(s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)))
    # (two branches may jump over one copy from different places: keep the widest of those that share their end)
    spans = [s for s in spans if not any(o != s and o[1] == s[1] and o[0] < s[0] for o in spans)]
    if len(spans) < 2:
        return [loop]
    return [[i for i in loop if not any(o != s and o[0] < i[0] < o[1] for o in spans)] for s in spans]


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
    """{kernel: classes of its row loop}; a kernel whose row has several copies gets one entry per copy as well (`name [copy k of n]`)"""
    with tempfile.TemporaryDirectory() as tmp:
        ks = kernels(code_object(obj, tmp))
    out = {}
    for n, i in ks.items():
        if fragment not in n:
            continue
        out[n] = classes(row_loop(i))
        copies = row_loop_copies(i, 6 if "tick_bgra_stream_cd" in n else 12)
        for k, c in enumerate(copies if len(copies) > 1 else []):
            out[f"{n[:40]} [copy {k + 1} of {len(copies)}]"] = classes(c)
    return out


if __name__ == "__main__":
    for name, c in sorted(count(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "").items()):
        print(name if "[copy " in name else name[:60], " ".join(f"{k}={v}" for k, v in c.items()))
