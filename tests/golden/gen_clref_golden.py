#!/usr/bin/env python3
"""Generate tests/golden/clref_vectors.npz — what the reference's own kernel strings, compiled for x86-64 (oracle/_ref/libclref.so),
compute for the cross-check cases of tests/test_oracle_golden.py (clref_layer_cases: every reference layer kernel on three geometries)
and tests/test_idle_kernels.py (snd_cases).  The tests compare the oracle with this recording wherever libclref.so cannot be built, and
check that libclref.so still reproduces it wherever it can.  Inputs are not stored: the cases rebuild them from their seeds.

Run where oracle/_ref/libclref.so builds (the reference tree present):  python tests/golden/gen_clref_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import test_idle_kernels as TI  # noqa: E402
import test_oracle_golden as TO  # noqa: E402
import util  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    if O.clref() is None or not hasattr(O.clref(), "clref_run_snd"):
        raise SystemExit("oracle/_ref/libclref.so (with snd_s16i_s16i) is not built: nothing to record")
    out = {}
    for key, kernel, src, c0, u in TO.clref_layer_cases():
        b = util.copy_image(c0)
        assert O.run_clref(kernel, b, src, u) == 0, key
        for i, p in enumerate(b):
            out[f"{key}/out{i}"] = p
    for name, out0, ins, gains, fades in TI.snd_cases():
        b = out0.copy()
        assert O.clref_snd_s16i_s16i(b, ins, O.snd_uniforms(gains, fades)) == 0, name
        out[f"snd/{name}"] = b
    np.savez_compressed(TO.CLREF_GOLD, **out)
    print(f"{TO.CLREF_GOLD}: {len(out)} arrays, {TO.CLREF_GOLD.stat().st_size} bytes")


if __name__ == "__main__":
    main()
