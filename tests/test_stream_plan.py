"""tick_bgra_stream's launch plan on the CPU: swiftvideo_amd/csrc/stream_plan.h — the planner launch_bgra_stream asks and the decode stream_body runs
— compiled with tests/cpp/test_stream_plan.cpp, which walks every (block, wave) of every plan: each (tick, strip, canvas row) covered exactly
once, phases that begin at multiples of 8 blocks, at most four of them and never taller than the one before, the grid the sum of the
rounded phases, one phase = today's rule and today's map (both restated there), a forced CHV_STREAM_ROWS = one phase.  The same program
runs once more, stand-alone, under the address and undefined-behaviour sanitizers.  The switch and the counter are asked of the built library."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "swiftvideo_amd" / "csrc"
SRC = ROOT / "tests" / "cpp" / "test_stream_plan.cpp"


def test_every_plan_covers_every_row_once(tmp_path):
    exe = tmp_path / "test_stream_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(SRC), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_same_under_sanitizers(tmp_path):
    exe = tmp_path / "test_stream_plan_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           f"-I{CSRC}", str(SRC), "-o", str(exe)])
    out = subprocess.run([str(exe), "quick"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_new_header_does_not_name_the_carry_launcher():
    assert "launch_bgra_stream_carry" not in (CSRC / "stream_plan.h").read_text()


def test_switch_and_counter_are_known_to_the_library(built):
    from swiftvideo_amd import chipvideo as cv
    try:
        for v in ("0", "1", "40", "160"):
            cv.set_switch("CHV_STREAM_PLAN", v)
    finally:
        cv.set_switch("CHV_STREAM_PLAN", None)
    assert cv.get_counter("stream_phased_launches") >= 0
