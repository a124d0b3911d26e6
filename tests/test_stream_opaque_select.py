"""Which launches of tick_bgra_stream take the opaque-bottom kernels: swiftvideo_amd/csrc/stream_select.h, the predicate launch_bgra_stream
asks, compiled for the CPU with tests/cpp/test_stream_select.cpp — only a bottom layer whose opacity is bit-equal to 1.0f in EVERY tick,
two layers or more, and the switch on; 0.99999994f, a one-layer tick, a batch in which one tick differs and CHV_STREAM_OPAQUE=0 all keep
the general kernels.  The switch and the launch counter are asked of the built library (no GPU needed for either)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_selection_predicate(tmp_path):
    exe = tmp_path / "test_stream_select"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'swiftvideo_amd' / 'csrc'}",
                           str(ROOT / "tests" / "cpp" / "test_stream_select.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_only_the_stream_unit_names_the_new_launcher():
    """chipvideo.cpp, geom_store.cpp and tick_route.cpp must link without the kernel units (tests/stubhip): launch_bgra_stream is the only caller"""
    for other in ("chipvideo.cpp", "geom_store.cpp", "tick_route.cpp", "kernels_fast.hip.cpp"):
        assert "launch_bgra_stream_opaque" not in (ROOT / "swiftvideo_amd" / "csrc" / other).read_text(), other


def test_switch_and_counter_are_known_to_the_library(built):
    from swiftvideo_amd import chipvideo as cv
    try:
        cv.set_switch("CHV_STREAM_OPAQUE", "0")
        cv.set_switch("CHV_STREAM_OPAQUE", "1")
    finally:
        cv.set_switch("CHV_STREAM_OPAQUE", None)
    assert cv.get_counter("stream_opaque_launches") >= 0
