"""The table of convolution forms (csrc/dt_conv_forms.h) against the expressions it replaced, without a GPU.

tests/host_sanitize/conv_forms_check.cpp is plain C++: it includes the header, holds the earlier hand-written expressions
(chunks per step, dynamic LDS per picture width, LDS limit, staging reach, epilogue stage and second stage, which
(kind, tile) exist) and compares them with the members of every form for W = 1..64.  It does the same for the
padded-channel map of the weight packs (conv_real_channel) against the three packers' earlier expressions, for every cin in
1..130 and every concat split: each real channel exactly once, -1 everywhere else.  Built here with the host compiler
under AddressSanitizer and UndefinedBehaviorSanitizer, then run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distillation_trajectories_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "host_sanitize", "conv_forms_check.cpp")


def _host_compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler is installed")
def test_forms_agree_with_the_expressions_they_replaced(tmp_path):
    exe = str(tmp_path / "conv_forms_check")
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-I", CSRC, CHECK, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    report = r.stdout[-6000:] + "\n" + r.stderr[-6000:]
    print(r.stdout[-300:])
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, report
    assert r.returncode == 0 and "conv forms ok" in r.stdout and " 0 mismatches" in r.stdout, report
