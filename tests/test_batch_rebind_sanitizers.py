"""chv_batch_rebind's host logic (swiftvideo_amd/csrc/chipvideo.cpp: validation, the per-slot buffers and dependencies, the pinned lists and their
events, the block's event) compiled for the CPU against the stand-in HIP runtime whose streams execute LAZILY (tests/stubhip/), with a stand-in
scatter launcher that writes the addresses into the stub's "device" block when the stream gets to it, and driven by
tests/stubhip/rebind_stress.cpp under AddressSanitizer + UBSan and under ThreadSanitizer: rotating rings over thousands of rebinds, buffers that
were rebound away freed once their runs have drained, an injected launch failure in the scatter, destroy with a rebind in flight and the pooled
block taken again, both mechanisms, three contexts, eight threads with a context and a batch each.  Every stub launch is an ordinary closure."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
STUB = ROOT / "tests" / "stubhip"
OUT = STUB / "_build"
CSRC = ROOT / "swiftvideo_amd" / "csrc"


def _build(kind):
    OUT.mkdir(exist_ok=True)
    exe = OUT / f"rebind_stress_{kind}"
    srcs = [CSRC / "chipvideo.cpp", CSRC / "geom_store.cpp", CSRC / "rebind.h", CSRC / "device_types.h", CSRC / "geom_cache.h", CSRC / "switches.h",
            ROOT / "include" / "chipvideo.h", STUB / "stub_runtime.cpp", STUB / "stub_launchers.cpp", STUB / "stub_rebind_launcher.cpp",
            STUB / "rebind_stress.cpp", STUB / "hip" / "hip_runtime.h", STUB / "build_rebind.sh"]
    if not exe.exists() or exe.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
        subprocess.check_call(["bash", str(STUB / "build_rebind.sh"), kind, str(exe)])
    return exe


@pytest.mark.parametrize("kind", ["address", "thread"])
def test_batch_rebind_host_logic_under_sanitizers(kind):
    exe = _build(kind)
    env = dict(os.environ, STUBHIP_DEVICES="2", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1")
    for k in list(env):
        if k.startswith("CHV_"):
            del env[k]
    out = subprocess.run([str(exe), "8"], capture_output=True, text=True, env=env, timeout=900)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "rebind_stress: ok" in text, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]


def test_the_host_units_link_without_the_scatter_launcher():
    """tests/stubhip/build.sh (the existing sanitizer build) has no unit that defines the launcher: chipvideo.cpp reaches it through a pointer it
    owns, null meaning the whole-block copy"""
    text = (CSRC / "chipvideo.cpp").read_text()
    assert "register_rebind_launcher" in text and "launch_batch_rebind" not in text
    assert "stub_rebind_launcher" not in (STUB / "build.sh").read_text()
