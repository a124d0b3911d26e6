"""Builds and runs tests/cpp/test_lanczos_hbd.cpp: the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) taking 10-bit decoder frames
(p010, y420p10) into nv12 and y420p pictures with Lanczos-3 — a ladder of three rungs of two pictures in two launches, the bytes of the six
single calls; luma the code over four at equal sizes; PictureFilter with convertHighBitDepth — and refusing malformed calls."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "tests" / "cpp" / "test_lanczos_hbd"


def _build():
    src = ROOT / "tests" / "cpp" / "test_lanczos_hbd.cpp"
    hdr = ROOT / "swiftvideo_amd" / "host" / "swiftvideo_hip.hpp"
    lib = ROOT / "swiftvideo_amd" / "libchipvideo.so"
    if EXE.exists() and EXE.stat().st_mtime > max(src.stat().st_mtime, hdr.stat().st_mtime, lib.stat().st_mtime):
        return
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-o", str(EXE), str(src), f"-L{ROOT / 'swiftvideo_amd'}", "-lchipvideo",
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", f"-Wl,-rpath,{ROOT / 'swiftvideo_amd'}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)


def test_cpp_lanczos_hbd_builds(built):
    """the mirror's overloads compile and link against the library (no device needed)"""
    _build()
    assert EXE.exists()


def run():
    """the program on the device; a case of tests/test_scale_lanczos_hbd_gpu.py's table"""
    _build()
    out = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "test_lanczos_hbd: ok" in out.stdout, out.stdout + out.stderr
