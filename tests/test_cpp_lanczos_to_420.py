"""Builds and runs tests/cpp/test_lanczos_to_420.cpp: the C++ host mirror (swiftvideo_amd/host/swiftvideo_hip.hpp) taking decoder frames of the
five formats nv21, y422p, y444p, yuvs and zvuy into nv12 and y420p pictures with Lanczos-3 — a ladder of three rungs of two pictures in two
launches, the bytes of the six single calls; luma an exact copy or unpack at equal sizes; PictureFilter with convertDecoderFormats — and refusing
malformed calls."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "tests" / "cpp" / "test_lanczos_to_420"


def _build():
    src = ROOT / "tests" / "cpp" / "test_lanczos_to_420.cpp"
    hdr = ROOT / "swiftvideo_amd" / "host" / "swiftvideo_hip.hpp"
    lib = ROOT / "swiftvideo_amd" / "libchipvideo.so"
    if EXE.exists() and EXE.stat().st_mtime > max(src.stat().st_mtime, hdr.stat().st_mtime, lib.stat().st_mtime):
        return
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-o", str(EXE), str(src), f"-L{ROOT / 'swiftvideo_amd'}", "-lchipvideo",
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", f"-Wl,-rpath,{ROOT / 'swiftvideo_amd'}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)


def test_cpp_lanczos_to_420_builds(built):
    """the mirror's overloads compile and link against the library (no device needed)"""
    _build()
    assert EXE.exists()


def run():
    """the program on the device; a case of tests/test_gpu_lanczos_to_420.py's table"""
    _build()
    out = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "test_lanczos_to_420: ok" in out.stdout, out.stdout + out.stderr
