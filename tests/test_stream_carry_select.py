"""Which opaque-bottom launches of tick_bgra_stream take the chroma-carry kernels: swiftvideo_amd/csrc/stream_select.h, the predicate
launch_bgra_stream_opaque asks, compiled for the CPU with tests/cpp/test_stream_carry_select.cpp — NV12 (not planar), a batch (not the by-value
lone tick), the switch on, and at most ONE chroma row per canvas row in every tick: both sides of that boundary, computed from the layer's
matrices and its chroma plane's height.  The switch and the launch counter are asked of the built library (no GPU needed for either)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "swiftvideo_amd" / "csrc"


def test_selection_predicate(tmp_path):
    exe = tmp_path / "test_stream_carry_select"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}",
                           str(ROOT / "tests" / "cpp" / "test_stream_carry_select.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_only_the_stream_units_name_the_new_launcher():
    """chipvideo.cpp and geom_store.cpp must link without the kernel units (tests/stubhip): the opaque-bottom unit is the only caller"""
    named = sorted(p.name for p in CSRC.iterdir() if p.suffix in (".cpp", ".h", ".inc") and "launch_bgra_stream_carry" in p.read_text())
    assert named == ["kernels_stream_carry.hip.cpp", "kernels_stream_opq.hip.cpp"], named
    stub = ROOT / "tests" / "stubhip"
    assert not any("launch_bgra_stream_carry" in p.read_text() for p in stub.rglob("*") if p.is_file() and p.suffix in (".cpp", ".h", ".sh"))


def test_switch_and_counter_are_known_to_the_library(built):
    from swiftvideo_amd import chipvideo as cv
    try:
        cv.set_switch("CHV_STREAM_CARRY", "0")
        cv.set_switch("CHV_STREAM_CARRY", "1")
    finally:
        cv.set_switch("CHV_STREAM_CARRY", None)
    assert cv.get_counter("stream_carry_launches") >= 0
    assert cv.get_counter("stream_opaque_launches") >= 0
