"""The host path of chv_scale_lanczos_hbd_to_420 / chv_scale_lanczos_hbd_to_420_ladder (swiftvideo_amd/csrc/chipvideo.cpp: validation of the
whole list with the evenness rule of 16-bit planes, dependencies, two tables per logical image per rung from the shared cache held until the
last launch is enqueued, the descriptor ring across chunk boundaries with records of n_rungs x target planes + 2 or 3 source planes, the launch
counter) compiled for the CPU against the stand-in HIP runtime whose streams execute LAZILY (tests/stubhip/), with a stand-in launcher that
makes one or two "launches" per chunk, reads the ends of every table and touches every plane's ends — a source plane's as 16-bit words — when
the stream gets to it, and driven by tests/stubhip/lanczos_hbd_stress.cpp — a stand-alone program — under AddressSanitizer + UBSan and under
ThreadSanitizer: every refusal, lists longer than a chunk, ladders of eight fresh geometries churning the table cache, an injected failure of
the second of two launches, several threads with a context each while two more free and re-create pictures, and the build without this
family's launcher.  Nothing here is loaded into Python and nothing is preloaded."""
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
    exe = OUT / f"lanczos_hbd_stress_{kind}"
    srcs = [CSRC / "chipvideo.cpp", CSRC / "geom_store.cpp", CSRC / "lanczos_hbd.h", CSRC / "lanczos_route.h", CSRC / "lanczos_420.h", CSRC / "lanczos_to_420.h",
            CSRC / "lanczos_planar_ladder.h", CSRC / "lanczos_ladder_grid.h", CSRC / "lanczos_planar.h", CSRC / "device_types.h", CSRC / "switches.h",
            ROOT / "include" / "chipvideo.h", STUB / "stub_runtime.cpp", STUB / "stub_lanczos_refuses.h", STUB / "stub_launchers.cpp",
            STUB / "stub_lanczos_hbd_launcher.cpp", STUB / "stub_lanczos_to_420_launcher.cpp", STUB / "stub_lanczos_420_launcher.cpp",
            STUB / "stub_lanczos_planar_ladder_launcher.cpp", STUB / "stub_lanczos_planar_launcher.cpp", STUB / "lanczos_hbd_stress.cpp",
            STUB / "hip" / "hip_runtime.h", STUB / "build_lanczos_hbd.sh"]
    if not exe.exists() or exe.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
        subprocess.check_call(["bash", str(STUB / "build_lanczos_hbd.sh"), kind, str(exe)])
    return exe


def _env():
    env = dict(os.environ, STUBHIP_DEVICES="2", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1")
    for k in list(env):
        if k.startswith("CHV_"):
            del env[k]
    return env


@pytest.mark.parametrize("kind", ["address", "thread"])
def test_lanczos_hbd_host_logic_under_sanitizers(kind):
    exe = _build(kind)
    out = subprocess.run([str(exe), "6"], capture_output=True, text=True, env=_env(), timeout=900)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "lanczos_hbd_stress: ok" in text, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]


def test_without_a_launcher_the_entries_are_not_implemented_after_validation():
    """the host units without the unit that defines this family's launcher: chipvideo.cpp reaches it through a pointer it owns, null meaning
    CHV_ERR_NOT_IMPLEMENTED, after validation"""
    text = (CSRC / "chipvideo.cpp").read_text()
    assert "register_lanczos_hbd_launcher" in text and "launch_lanczos_hbd" not in text
    assert "lanczos_hbd" not in (STUB / "build.sh").read_text()
    exe = _build("none")
    out = subprocess.run([str(exe), "unregistered"], capture_output=True, text=True, env=_env(), timeout=300)
    assert out.returncode == 0 and "not implemented without a launcher, ok" in out.stdout, (out.stdout + out.stderr)[-4000:]
