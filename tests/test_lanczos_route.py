"""The integer rules of the Lanczos units' host halves on the CPU: swiftvideo_amd/csrc/lanczos_route.h — the tap class, the rows-per-wave rule, the
160 KB refusal and the strip-route rule — compiled with tests/cpp/test_lanczos_route.cpp, which holds the answers of the per-unit copies these
functions replaced as literal tables (tap counts 1 .. 23, launches of 0 to 2^40 rows, scales from 1:8 to 30:1 on each axis and the bound itself)
and pins planar_strip_route to x420_strip_route on same-format geometries.  The same program runs once more, stand-alone, under the address and
undefined-behaviour sanitizers."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "swiftvideo_amd" / "csrc"
SRC = ROOT / "tests" / "cpp" / "test_lanczos_route.cpp"


def test_the_shared_rules_answer_as_the_units_did(tmp_path):
    exe = tmp_path / "test_lanczos_route"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(SRC), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_same_under_sanitizers(tmp_path):
    exe = tmp_path / "test_lanczos_route_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           f"-I{CSRC}", str(SRC), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_header_needs_no_hip():
    text = (CSRC / "lanczos_route.h").read_text()
    assert "hip_runtime" not in text and "asm" not in text
