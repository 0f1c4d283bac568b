"""Host-side AddressSanitizer + UndefinedBehaviorSanitizer run of the library (VERDICT r02 missing 4).

csrc/_build/dt_host_sanitize (built by ``csrc/build.py::build_sanitizer_driver``, i.e. by ``__graft_entry__.build()``) links
the library's own sources with the HOST code instrumented and walks weight packing, launch plans, forwards,
the sampler loops (plain, hipGraph replay, mixed batch), the profiler, the metric launchers and the argument-error paths
through the C ABI (tests/host_sanitize/driver.cpp).  Device code is not instrumented: GPU ASan is unavailable on this pool."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "distillation_trajectories_amd", "csrc", "_build", "dt_host_sanitize")


@pytest.mark.gpu
def test_host_code_is_clean_under_asan_and_ubsan():
    if not os.path.exists(DRIVER):
        from distillation_trajectories_amd.csrc.build import build_sanitizer_driver
        build_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([DRIVER], capture_output=True, text=True, env=env, timeout=600)
    report = r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, report
    assert r.returncode == 0 and "driver ok" in r.stdout, report


def test_sanitizer_driver_source_covers_every_export():
    """The driver calls every function include/dt_hip.h declares (so that a new entry point is not forgotten)."""
    import re
    header = open(os.path.join(ROOT, "include", "dt_hip.h")).read()
    names = set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", header)) - {"dt_unet"}
    src = open(os.path.join(ROOT, "tests", "host_sanitize", "driver.cpp")).read()
    missing = sorted(n for n in names if n + "(" not in src)
    assert not missing, missing
