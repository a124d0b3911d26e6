"""The grid of a Lanczos ladder launch on the CPU: swiftvideo_amd/csrc/lanczos_ladder_grid.h — the order the launchers ask for and the scan and
numbering the kernels run — compiled with tests/cpp/test_ladder_grid.cpp, which walks every block of ladders of 1 to 8 rungs with the strip
route's padding of 8 and the tile route's of 1: each (rung, item) the work of exactly one live block, the dead blocks the grid minus the work,
ranges that begin on multiples of the padding, first[] closed with INT_MAX, largest rung first with ties in the caller's order, and the
30-bit refusal.  The same program runs once more, stand-alone, under the address and undefined-behaviour sanitizers."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "swiftvideo_amd" / "csrc"
SRC = ROOT / "tests" / "cpp" / "test_ladder_grid.cpp"


def test_every_ladder_grid_covers_every_item_once(tmp_path):
    exe = tmp_path / "test_ladder_grid"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(SRC), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_same_under_sanitizers(tmp_path):
    exe = tmp_path / "test_ladder_grid_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           f"-I{CSRC}", str(SRC), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_header_needs_no_hip():
    text = (CSRC / "lanczos_ladder_grid.h").read_text()
    assert "hip_runtime" not in text and "asm" not in text
