"""Builds and runs tests/cpp/test_lanczos_rgb_ladder.cpp: the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) making every rendition
of a list of BGRA or RGBA pictures with one call — four rungs over two pictures in two launches, the bytes of the eight single calls — and
refusing malformed ladders."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "tests" / "cpp" / "test_lanczos_rgb_ladder"


def _build():
    src = ROOT / "tests" / "cpp" / "test_lanczos_rgb_ladder.cpp"
    hdr = ROOT / "swiftvideo_amd" / "host" / "swiftvideo_hip.hpp"
    lib = ROOT / "swiftvideo_amd" / "libchipvideo.so"
    if EXE.exists() and EXE.stat().st_mtime > max(src.stat().st_mtime, hdr.stat().st_mtime, lib.stat().st_mtime):
        return
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-o", str(EXE), str(src), f"-L{ROOT / 'swiftvideo_amd'}", "-lchipvideo",
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", f"-Wl,-rpath,{ROOT / 'swiftvideo_amd'}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)


def test_cpp_lanczos_rgb_ladder_builds(built):
    """the mirror's overload compiles and links against the library (no device needed)"""
    _build()
    assert EXE.exists()


@pytest.mark.gpu
def test_cpp_lanczos_rgb_ladder_equals_the_single_calls(built):
    _build()
    out = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "test_lanczos_rgb_ladder: ok" in out.stdout, out.stdout + out.stderr
