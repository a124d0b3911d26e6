"""Which kernel runs a compositing tick, on the CPU: swiftvideo_amd/csrc/tick_route.cpp (select_fast_path and what it asks, split_stream_prefix,
select_tail_path, wave_layers_by_value, the four *_eligible predicates, plan_wave_layers through wave_geom_config), compiled by
g++ alone with tests/cpp/test_tick_route.cpp.  That program builds small descriptors in code, sets the switches per case through its own
chv::switches(), and holds, as literal tables (tests/cpp/tick_route_answers.inc, tick_route_ys_round.inc), what the rules answered while they
lived in the host halves of four kernel units: every threshold of section 5 with a case on each side, the bound itself where it is a double.
The same program runs once more, stand-alone, under the address and undefined-behaviour sanitizers."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "swiftvideo_amd" / "csrc"
SRCS = [str(ROOT / "tests" / "cpp" / "test_tick_route.cpp"), str(CSRC / "tick_route.cpp")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"]


def test_the_route_rules_answer_as_the_kernel_units_did(tmp_path):
    exe = tmp_path / "test_tick_route"
    subprocess.check_call(["g++", "-O2", *FLAGS, *SRCS, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_same_under_sanitizers(tmp_path):
    exe = tmp_path / "test_tick_route_san"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *FLAGS, *SRCS, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_unit_needs_no_hip():
    for name in ("tick_route.h", "tick_route.cpp"):
        text = (CSRC / name).read_text()
        assert "hip_runtime" not in text and "asm" not in text, name
        assert not re.search(r'#include\s+"[^"]*\.hip\.(h|inc)"', text), name
