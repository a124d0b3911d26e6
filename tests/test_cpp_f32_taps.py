"""Builds and runs tests/cpp/test_f32_taps.cpp: the identity that lets tick_bgra_stream_cd feed its taps to the f32 multiplier as binary32
denormals — the scaled chain plus fma(S, 2^22, m) against the reference chain plus m, bit for bit, over the weight grid
{0, 2^-24, 2^-23, 1/4, 1/3, 1/2, 1 - 2^-24, 1}^2 with every byte in every tap position (the others at 0 and at 255), 10^6 random pairs
with random bytes, and the nine conversion constants of the absorbed matrices.  No GPU, no library."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_scaled_chain_equals_reference_chain_bit_for_bit(tmp_path):
    exe = tmp_path / "test_f32_taps"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           str(ROOT / "tests" / "cpp" / "test_f32_taps.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout + out.stderr
    # the three constants of each absorbed matrix are the table's (swiftvideo_amd/csrc/pixel_math.hip.h)
    table = (ROOT / "swiftvideo_amd" / "csrc" / "pixel_math.hip.h").read_text()
    src = (ROOT / "tests" / "cpp" / "test_f32_taps.cpp").read_text()
    for m in ("10041594.0f, 13672062.0f, 9933686.0f", "8659076.0f, 15468090.0f, 11137308.0f", "8400986.0f, -15564928.0f, -9977984.0f"):
        assert m in table and m in src
