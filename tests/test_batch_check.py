"""The argument checks of the five batch entries (csrc/dt_batch.h) against the condition lists they replaced, without a GPU.

tests/host_sanitize/batch_check.cpp is plain C++: it includes the header, holds the earlier condition lists of
dt_unet_forward, dt_unet_forward_mixed, dt_sample_trajectory, dt_sample_trajectory_mixed and dt_sample_trajectory_masked
verbatim (with the tests at the head of forward_impl and sample_loop that followed them, down to the workspace-size test) and
compares each with the header's status function over the grid rule {-1, 0, 2, 3} x B 0..5 x n_pass 0..3 x B_single -1..6 x
tb_div 0..6 x four picture sizes x n_steps {-1, 0, 2} x share_enc1 off / on x every pointer null in turn x mask, known and
traj off 16-byte alignment in turn.  Built here with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer, then run.

A grid that only produced errors would prove nothing: every status the old text of an entry can return before it sizes the
workspace must occur, DT_OK included.  dt_unet_forward cannot return DT_E_ARG there (its rows are B * n_pass, which B always
divides, and rows that tb_div does not divide are refused after the workspace test, on the fused path only)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distillation_trajectories_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "host_sanitize", "batch_check.cpp")

REACHABLE = {
    "dt_unet_forward": {"DT_OK", "DT_E_NULL", "DT_E_SHAPE"},
    "dt_unet_forward_mixed": {"DT_OK", "DT_E_NULL", "DT_E_SHAPE", "DT_E_ARG"},
    "dt_sample_trajectory": {"DT_OK", "DT_E_NULL", "DT_E_SHAPE", "DT_E_ARG"},
    "dt_sample_trajectory_mixed": {"DT_OK", "DT_E_NULL", "DT_E_SHAPE", "DT_E_ARG"},
    "dt_sample_trajectory_masked": {"DT_OK", "DT_E_NULL", "DT_E_SHAPE", "DT_E_ARG"},
}


def _host_compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler is installed")
def test_status_functions_agree_with_the_condition_lists_they_replaced(tmp_path):
    exe = str(tmp_path / "batch_check")
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-I", CSRC, CHECK, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    report = r.stdout[-6000:] + "\n" + r.stderr[-6000:]
    print(r.stdout[-1200:])
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, report
    assert r.returncode == 0 and "batch check ok" in r.stdout and " 0 mismatches" in r.stdout, report
    for entry, reachable in REACHABLE.items():
        line = re.search(rf"^{entry}:(.*)$", r.stdout, re.M)
        assert line, report
        counts = {name: int(n) for name, n in re.findall(r"(DT_\w+) (\d+)", line.group(1))}
        assert {name for name, n in counts.items() if n > 0} == reachable, (entry, counts)
