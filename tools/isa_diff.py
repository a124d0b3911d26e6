#!/usr/bin/env python3
"""tools/isa_diff.py [--rev REV] [-DFLAG ...] <stem> ... — is the gfx950 code of swiftvideo_amd/csrc/<stem>.hip.cpp what it was at REV
(default HEAD~)?  Both trees' units are compiled with the Makefile's own command line (plus the -D flags), the code objects unbundled as
tools/kernel_regs.py and tools/kernel_ops.py do, and compared symbol by symbol: `llvm-objdump -d --no-show-raw-insn` without the trailing
`// address:` comments, and the per-kernel metadata notes (registers, spills, scratch, LDS, kernarg size).  Prints the symbols that differ;
exit status 1 if any does.  For refactors of kernel source that must leave the device code alone."""
import re, shlex, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")
CSRC = "swiftvideo_amd/csrc"
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size", "uses_dynamic_stack")


def compile_unit(csrc, stem, extra, obj):
    """the object of <stem>.hip.cpp in the tree at `csrc`, by the command `make` would run there"""
    cmd = subprocess.run(["make", "-n", "-B", "-C", str(csrc), f"{stem}.hip.o"], check=True, capture_output=True, text=True).stdout
    cmd = [l for l in cmd.splitlines() if f"-c {stem}.hip.cpp" in l][-1]
    cmd = cmd.replace(f"-o {stem}.hip.o", f"-w -o {shlex.quote(str(obj))}") + " " + " ".join(shlex.quote(e) for e in extra)
    subprocess.run(cmd, shell=True, check=True, cwd=csrc)


def listing(obj):
    """({symbol: instruction text}, {kernel: metadata}) of a built object's gfx950 code"""
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        subprocess.run([LLVM / "llvm-objcopy", f"--dump-section=.hip_fatbin={d/'f'}", obj, d / "copy.o"], check=True)
        subprocess.run([LLVM / "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={d/'f'}", f"--output={d/'co'}"], check=True)
        dis = subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", d / "co"], check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([LLVM / "llvm-readelf", "--notes", d / "co"], check=True, capture_output=True, text=True).stdout
    parts = re.split(r"\n[0-9a-f]+ <([^>+]*)>:\n", dis)
    text = {name: "\n".join(re.sub(r"\s*//.*$", "", l) for l in body.splitlines() if l.strip()) for name, body in zip(parts[1::2], parts[2::2])}
    # amdhsa.kernels is a YAML list with every item's keys in alphabetical order (.name comes late): collect an item, key it by its .name when it ends
    meta, item, indent = {}, None, None
    def close():
        if item and ".name" in item:
            meta[item[".name"]] = {k: item["." + k] for k in META if "." + k in item}
    for line in notes.splitlines():
        body = line.lstrip(" ")
        at = len(line) - len(body)
        if body.startswith("amdhsa.kernels:"):
            indent = -1
        elif indent is not None and body:
            if indent == -1 and body.startswith("- "):
                indent = at
            if at < indent:
                close(); item, indent = None, None
            elif at == indent and body.startswith("- "):
                close(); item = {}
                body, at = body[2:], at + 2
            if item is not None and at == indent + 2:
                m = re.match(r"(\.\w+):\s*(\S*)", body)
                if m:
                    item[m.group(1)] = m.group(2)
    close()
    return text, meta


def differences(old, new):
    """names whose text / metadata differ between two listings, with what differs"""
    out = []
    for what, a, b in (("text", old[0], new[0]), ("metadata", old[1], new[1])):
        for name in sorted(set(a) | set(b)):
            if name not in a or name not in b:
                out.append(f"{what}: {name}: only in the {'new' if name in b else 'old'} object")
            elif a[name] != b[name]:
                if what == "text":
                    la, lb = a[name].splitlines(), b[name].splitlines()
                    first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
                    out.append(f"text: {name}: {len(la)} -> {len(lb)} lines, first difference at line {first}")
                else:
                    out.append(f"metadata: {name}: " + ", ".join(f"{k} {a[name].get(k)} -> {b[name].get(k)}" for k in META if a[name].get(k) != b[name].get(k)))
    return out


def main():
    args, rev = sys.argv[1:], "HEAD~"
    if args[:1] == ["--rev"]:
        rev, args = args[1], args[2:]
    extra, stems = [a for a in args if a.startswith("-")], [a for a in args if not a.startswith("-")]
    if not stems:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", rev, CSRC, "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", str(d)], input=tar, check=True)
        jobs = [(side, tree / CSRC, s, d / f"{side}_{s}.o") for s in stems for side, tree in (("old", d), ("new", ROOT))]
        with ThreadPoolExecutor(max_workers=4) as pool:
            list(pool.map(lambda j: compile_unit(j[1], j[2], extra, j[3]), jobs))
        bad = 0
        for s in stems:
            old, new = listing(d / f"old_{s}.o"), listing(d / f"new_{s}.o")
            diff = differences(old, new)
            bad += len(diff)
            lines = sum(t.count("\n") + 1 for t in new[0].values())
            print(f"{s} vs {rev}{' ' + ' '.join(extra) if extra else ''}: {len(new[0])} symbols, {len(new[1])} kernels, {lines} instruction lines, {len(diff)} differing")
            for l in diff:
                print("  " + l)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
