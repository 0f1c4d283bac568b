"""The row arithmetic of the convolution kernels (csrc/dt_conv_rows.h) against plain `/` and `%`, without a GPU.

tests/host_sanitize/conv_row_math_check.cpp is plain C++: it includes the header and compares every helper the kernels
use -- time-bias row (single output, both passes of a dual-output launch with and without single-pass rows in front),
picture, (y, x), border class, tap mask, pooled row, pooling window, the split-K pass's window row, the image of enc1's
skip -- with the division it replaces: every row m in [0, 2 BM + 7) for BM in {64, 128, 256}, pictures 1x1, 2x2, 4x4, 8x8,
16x16, 6x6, 4x6, 3x5, m_per_tb in {HW, 3 HW, BM, BM + HW, the whole launch} and dup_skip in {0, 256}; and the
multiply-shift pair itself for every divisor up to 1100 and at both ends of the 31-bit range.  Built here with the host
compiler under AddressSanitizer and UndefinedBehaviorSanitizer, then run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distillation_trajectories_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "host_sanitize", "conv_row_math_check.cpp")


def _host_compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler is installed")
def test_row_math_agrees_with_division(tmp_path):
    exe = str(tmp_path / "conv_row_math_check")
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-I", CSRC, CHECK, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    report = r.stdout[-6000:] + "\n" + r.stderr[-6000:]
    print(r.stdout[-300:])
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, report
    assert r.returncode == 0 and "conv row math ok" in r.stdout and " 0 mismatches" in r.stdout, report
