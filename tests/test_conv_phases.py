"""Instruction counts of the convolution kernels by phase, as compiled: tools/kernel_phases.py against two committed reports.

profiles/conv_phases_parent.txt is the report of the commit before the row arithmetic went to multiply-shift pairs
(csrc/dt_conv_rows.h): no kernel may have more instructions before its first MFMA, after its last MFMA or in its main loop
than it records, nor more MFMAs in that loop, more VGPRs or more spilled VGPRs.  profiles/conv_phases.txt is the report of
that change; later changes are held to its phase counts (a prologue or epilogue that grows again is a finding), and the
K-split strip forms and every split-K sum kernel to its division count (the one left is the grid-stride index of the sum
kernel on channel counts that are no power of two).  A change that lowers the counts commits the new report with it."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARENT = os.path.join(ROOT, "profiles", "conv_phases_parent.txt")
CURRENT = os.path.join(ROOT, "profiles", "conv_phases.txt")


def _have_hipcc():
    return os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc") is not None or os.path.exists(os.environ.get("HIPCC", "/nonexistent"))


@pytest.fixture(scope="module")
def phases():
    import kernel_phases
    report = kernel_phases.report()
    text = kernel_phases.format_report(report)
    print(text)
    got = {}
    for _, kernels in report:
        got.update(kernels)
    assert kernel_phases.parse_report(text) == {k: {f: v[f] for f in kernel_phases.FIELDS} for k, v in got.items()}
    return kernel_phases, got


def _worse(got, want, fields):
    bad = {}
    for name, rec in sorted(want.items()):
        assert name in got, f"{name} is not compiled any more"
        over = {f: (rec[f], got[name][f]) for f in fields if got[name][f] > rec[f]}
        if over:
            bad[name] = over
    return bad


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed")
def test_no_phase_grew_against_the_parent(phases):
    tool, got = phases
    with open(PARENT) as f:
        parent = tool.parse_report(f.read())
    assert len(parent) == 33 and sorted(parent) == sorted(got), sorted(set(parent) ^ set(got))
    bad = _worse(got, parent, ("pre", "post", "loop", "loop_mfma", "vgprs", "spill"))
    assert not bad, f"(parent, now) per kernel and field: {bad}"


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed")
def test_phases_stay_where_the_row_arithmetic_change_left_them(phases):
    tool, got = phases
    with open(CURRENT) as f:
        current = tool.parse_report(f.read())
    assert sorted(current) == sorted(got), sorted(set(current) ^ set(got))
    bad = _worse(got, current, ("pre", "post", "loop", "loop_mfma", "div", "vgprs", "spill"))
    assert not bad, f"(profiles/conv_phases.txt, now) per kernel and field: {bad}"
    # what the change bought, so that a report committed by mistake from the wrong tree is noticed
    with open(PARENT) as f:
        parent = tool.parse_report(f.read())
    for name, rec in current.items():
        assert rec["div"] <= 2 and rec["div_post"] == 0, (name, rec)
        if rec["mfma"]:
            assert rec["post"] * 10 <= parent[name]["post"] * 9, (name, rec["post"], parent[name]["post"])
