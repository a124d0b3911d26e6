"""The host path of the 4:2:0 Lanczos families (swiftvideo_amd/csrc/chipvideo.cpp: per-plane validation, dependencies, up to four tables from
the shared cache held until the launch is enqueued, the descriptor ring of the batch entry) compiled for the CPU against the stand-in HIP
runtime whose streams execute LAZILY (tests/stubhip/), with a stand-in launcher that reads every table's ends and touches every plane's ends
when the stream gets to it, and driven by tests/stubhip/lanczos_planar_stress.cpp under AddressSanitizer + UBSan and under ThreadSanitizer:
singles and batches of 130 NV12 / y420p pictures, 70 geometries churning the table cache, refusals, an injected launch failure, several
threads with a context each while two more free and re-create pictures."""
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
    exe = OUT / f"lanczos_planar_stress_{kind}"
    srcs = [CSRC / "chipvideo.cpp", CSRC / "geom_store.cpp", CSRC / "lanczos_planar.h", CSRC / "rebind.h", CSRC / "device_types.h", CSRC / "geom_cache.h",
            CSRC / "switches.h", ROOT / "include" / "chipvideo.h", STUB / "stub_runtime.cpp", STUB / "stub_launchers.cpp",
            STUB / "stub_lanczos_planar_launcher.cpp", STUB / "lanczos_planar_stress.cpp", STUB / "hip" / "hip_runtime.h", STUB / "build_lanczos.sh"]
    if not exe.exists() or exe.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
        subprocess.check_call(["bash", str(STUB / "build_lanczos.sh"), "planar", kind, str(exe)])
    return exe


def _env():
    env = dict(os.environ, STUBHIP_DEVICES="2", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1")
    for k in list(env):
        if k.startswith("CHV_"):
            del env[k]
    return env


@pytest.mark.parametrize("kind", ["address", "thread"])
def test_lanczos_planar_host_logic_under_sanitizers(kind):
    exe = _build(kind)
    out = subprocess.run([str(exe), "6"], capture_output=True, text=True, env=_env(), timeout=900)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "lanczos_planar_stress: ok" in text, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]


def test_without_a_launcher_the_yuv_families_are_not_implemented():
    """the host units as tests/stubhip/build.sh links them — no unit that defines the launcher: chipvideo.cpp reaches it through a pointer it
    owns, null meaning CHV_ERR_NOT_IMPLEMENTED for NV12 and y420p while the 4-component family runs as before"""
    text = (CSRC / "chipvideo.cpp").read_text()
    assert "register_lanczos_planar_launcher" in text and "launch_lanczos_planar" not in text
    assert "lanczos_planar" not in (STUB / "build.sh").read_text()
    exe = _build("none")
    out = subprocess.run([str(exe), "unregistered"], capture_output=True, text=True, env=_env(), timeout=300)
    assert out.returncode == 0 and "not implemented without a launcher, ok" in out.stdout, (out.stdout + out.stderr)[-4000:]


def test_the_existing_sanitizer_build_still_links(tmp_path):
    """tests/stubhip/build.sh, unchanged: chipvideo.cpp + stub_launchers.cpp and no kernel unit"""
    subprocess.check_call(["bash", str(STUB / "build.sh"), "address", str(tmp_path / "abi_stress_address")])
