"""Builds and runs tests/cpp/test_batch_rebind.cpp: the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) ticking a VideoMixerGroup that
keeps and rebinds its batches against one that builds a batch per tick — the same bytes, tick by tick."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "tests" / "cpp" / "test_batch_rebind"


def _build():
    src = ROOT / "tests" / "cpp" / "test_batch_rebind.cpp"
    hdr = ROOT / "swiftvideo_amd" / "host" / "swiftvideo_hip.hpp"
    lib = ROOT / "swiftvideo_amd" / "libchipvideo.so"
    if EXE.exists() and EXE.stat().st_mtime > max(src.stat().st_mtime, hdr.stat().st_mtime, lib.stat().st_mtime):
        return
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-o", str(EXE), str(src), f"-L{ROOT / 'swiftvideo_amd'}", "-lchipvideo",
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", f"-Wl,-rpath,{ROOT / 'swiftvideo_amd'}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)


def test_cpp_batch_rebind_builds(built):
    """the mirror's rebind and reuseBatches compile and link against the library (no device needed)"""
    _build()
    assert EXE.exists()


@pytest.mark.gpu
def test_cpp_group_with_kept_batches_equals_the_default_group(built):
    _build()
    out = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "test_batch_rebind: ok" in out.stdout, out.stdout + out.stderr
