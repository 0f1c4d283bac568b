"""The U-Net's geometry, weight-slab layout and workspace plan (csrc/dt_unet_layout.h) against the text they replaced, without a GPU.

tests/host_sanitize/unet_layout_check.cpp is plain C++: it includes the header, holds the geometry and offset part of
dt_unet_create and make_plan verbatim as ``before::`` and compares every geometry field, every slab offset, tb_cols, tb_stride,
the slab total and every Plan offset, H[j], W[j] and total over the grid channels 1..3 x temb_dim {2, 7, 64, 128} x share_enc1
off / on x 14 dims (the synthetic models at size factors 0.1, 0.25, 0.3, 0.4, 0.5 and 1.0, dims that are no multiples of 16,
dims with equal neighbours) x rows {1, 2, 5, 41, 82, 512, 4096} x five picture sizes.  Independently of the old text every
region of both layouts starts on a 256-byte boundary, lies inside the total and is disjoint from the others.  Built here with
the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer, then run.

A grid that only visited one kind of case would prove nothing: it must hold a block in 1..7 with an identity skip and one with
a 1x1 skip conv, blocks with rows * h * w on each side of kSplitMaxRows, and both values of share_enc1."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distillation_trajectories_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "host_sanitize", "unet_layout_check.cpp")


def _host_compiler():
    for name in ("g++", "clang++", "c++"):
        path = shutil.which(name)
        if path:
            return path
    return None


@pytest.mark.skipif(_host_compiler() is None, reason="no host C++ compiler is installed")
def test_layouts_agree_with_the_text_they_replaced(tmp_path):
    exe = str(tmp_path / "unet_layout_check")
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-I", CSRC, CHECK, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    report = r.stdout[-6000:] + "\n" + r.stderr[-6000:]
    print(r.stdout[-1200:])
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, report
    assert r.returncode == 0 and "unet layout check ok" in r.stdout, report
    assert re.search(r"compared \d+ values: 0 mismatches, 0 region faults", r.stdout), report

    def counts(pattern):
        m = re.search(pattern, r.stdout)
        assert m, report
        return [int(v) for v in m.groups()]

    models, shapes, refused = counts(r"models (\d+)  forward shapes (\d+)  refused descriptions (\d+)")
    assert models == 3 * 4 * 2 * 14 and shapes == models * 7 * 5 and refused == 6, report
    assert all(n > 0 for n in counts(r"has_res true (\d+)  has_res false (\d+)")), report
    assert all(n > 0 for n in counts(r"rows at most kSplitMaxRows (\d+)  above (\d+)")), report
    assert all(n > 0 for n in counts(r"share_enc1: on (\d+)  off (\d+)")), report
