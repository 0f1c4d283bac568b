"""Registers of the pair kernel, as the compiler reports them: tools/kernel_resources.py compiles csrc/dt_conv_strip_pair.hip
device-only for gfx950 (nothing is run, no GPU needed).  The pair kernel is the NH = 2 instantiation of the strip kernel
(csrc/dt_conv_strip_kernel.h), conv_strip_bf16x6_kernel<256,64,2,1,2>.  It runs as one workgroup of eight waves per CU, two
waves per SIMD: at most 256 VGPRs, no spilled VGPR and no scratch, so that nothing but LDS and the operand loads stands
between its MFMAs.  Its code object holds that one kernel, and the three other conv code objects
(tests/test_kernel_resources.py) hold no NH = 2 instantiation."""
import re

import pytest

from test_kernel_resources import _have_hipcc, _resources

KERNEL = "conv_strip_bf16x6_kernel<256,64,2,1,2>"


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed")
def test_pair_kernel_registers_and_scratch():
    res = _resources("dt_conv_strip_pair.hip")
    assert sorted(res) == [KERNEL], sorted(res)
    r = res[KERNEL]
    print(f"{KERNEL}: {r['vgprs']} VGPRs, {r['agprs']} AGPRs, {r['vgpr_spill']} spilled, {r['scratch_bytes']} B scratch, "
          f"occupancy {r['occupancy']}, {r['lds_bytes']} B static LDS")
    assert r["vgprs"] + r["agprs"] <= 256 and r["occupancy"] == 2, r
    assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0, r
    assert r["lds_bytes"] == 0, r                      # all of its LDS is dynamic (dt_conv_strip_pair.h)


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed")
def test_pinned_conv_code_objects_do_not_hold_the_pair_kernel():
    for src in ("dt_conv.hip", "dt_conv_bf16.hip", "dt_conv_strip.hip"):
        names = list(_resources(src))
        # every strip kernel there is an NH = 1 instantiation: <BM,BN,KC,WK,1>
        assert not [n for n in names if n.startswith("conv_strip_bf16x6_kernel<") and not re.search(r"<\d+,\d+,\d+,\d+,1>$", n)], src
