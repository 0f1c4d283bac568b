"""The pair kernel (csrc/dt_conv_strip_pair.hip) against the kernel it stands in for, and against float64.

A 256 x 64 launch of the K = 32 strip kind on a layer whose padded output channels are a multiple of 128 is served by
conv_strip_pair_bf16x6_kernel: one eight-wave workgroup walks two adjacent N tiles over one staged strip.  The order of the
operations behind an output element is conv_strip_bf16x6_kernel<256,64,2,1>'s, so for every pin below

  * the forward of a handle created under DT_NO_STRIP_PAIR=1 (the old kernel) and of a default handle (the pair kernel) agree
    bit for bit -- every block output and eps, under a NaN- and a 1e30-poisoned workspace;
  * the in-library profiler names the kernel that ran: the pair kernel under its own name on the default handle, never on the
    other one; a layer of 192 output channels (three N tiles) falls back to <256,64> on both;
  * the pinned block's output passes the float64 checks of tests/test_hip_conv_blocks.py (its helpers and tolerances,
    imported): |err| <= TAU * S elementwise, per-image relative L2 and RMS of err / S, zero padding channels.

Shapes are the smallest that reach each path: one pair (N = 128) and two (N = 256); 32 input channels (one chunk group) and
48 (three chunks: the zero chunk of the pack, in the 3x3 walk and in the folded skip walk); pictures of 16 x 16 and 8 x 8
(halo W) and 6 x 6 (halo W + 1, picture boundaries inside a 32-row fragment); M no multiple of 256 (five images of 8 x 8 in
two passes: 640 rows, the pass boundary inside a tile; 72 and 96 rows: one ragged tile); conv1 with a time-bias row per
sample; conv2 with the identity residual, with the folded 1x1 skip of one source and of the decoder's two-source concat;
enc1.conv2's dual output with the fused pool and the image skip on 1- and 3-channel images (head fusion off and on); split 2
through the slab sum.
"""
import contextlib
import io

import pytest
import torch
import torch.nn as nn

from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd._hip import check
from distillation_trajectories_amd.config import Config
from distillation_trajectories_amd.models import BLOCK_NAMES, Block, DiffusionUNet, block_channels
from distillation_trajectories_amd.synthetic import randomize_bn
from test_hip_conv_blocks import (C_TAU, POISONS, REL_L2, RMS_C, SLOT_NAMES, Case, Runner, bits, block_references, check_block,
                                  row_temb)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIR = "conv_strip_pair_bf16x6_kernel<256,128>"
OLD = "conv_strip_bf16x6_kernel<256,64>"
STRIP32 = 4          # KIND_STRIP2

# (name, image channels, dims, H, W, images, passes, tb_div, seed, [(block, slot, splits, fuse, served by the pair kernel)])
SHAPES = (
    # enc1.conv2: 3 images of 16 x 16 for both passes (n_dup = 2), pool and image skip; enc2 128 -> 128: identity residual,
    # time-bias row per sample, split 2; enc3 -> 256 channels: two pairs, 96 rows; dec1: the two-source concat
    ("A_c3_d128_128_256_256", 3, (128, 128, 256, 256), 16, 16, 3, 2, 1, 31,
     [(0, 2, 1, 0, True), (1, 1, 1, 0, True), (1, 1, 2, 0, True), (1, 2, 1, 0, True), (2, 1, 1, 0, True), (2, 2, 1, 1, True),
      (7, 1, 1, 0, True), (7, 1, 2, 0, True), (7, 2, 1, 1, True)]),
    # 1-channel images; enc2 has 192 output channels: three N tiles, which do not pair up
    ("B_c1_d128_192_128_128", 1, (128, 192, 128, 128), 16, 16, 3, 2, 3, 32,
     [(0, 2, 1, 0, True), (1, 1, 1, 0, False), (1, 2, 1, 1, False)]),
    # 32 input channels: one chunk group; five images of 8 x 8 in two passes: 640 rows
    ("C_c3_d32_128_128_128", 3, (32, 128, 128, 128), 16, 16, 5, 2, 1, 33,
     [(1, 1, 1, 0, True), (1, 2, 1, 1, True), (1, 2, 1, 0, True)]),
    # 48 input channels: three chunks in steps of two
    ("D_c3_d48_128_128_128", 3, (48, 128, 128, 128), 16, 16, 5, 2, 5, 34,
     [(1, 1, 1, 0, True), (1, 2, 1, 1, True)]),
    # 48 x 48 images: enc4 and dec3 see 6 x 6 pictures (72 rows), enc3 12 x 12, enc2 24 x 24
    ("E_c3_d32_128_128_128_48px", 3, (32, 128, 128, 128), 48, 48, 1, 2, 1, 35,
     [(3, 1, 1, 0, True), (3, 2, 1, 0, True), (5, 1, 1, 0, True), (5, 2, 1, 1, True), (2, 1, 1, 0, True), (1, 2, 1, 1, True)]),
)


def custom_state_dict(channels, dims, seed):
    """a seeded U-Net of arbitrary widths: models.DiffusionUNet's keys, its blocks rebuilt for `dims`"""
    cfg = Config()
    cfg.image_size = 16
    cfg.channels = channels
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = DiffusionUNet(cfg, 0.25)
    for name, (cin, cout) in zip(BLOCK_NAMES, block_channels(channels, list(dims))):
        setattr(m, name, Block(cin, cout, m.time_emb_dim))
    m.final = nn.Conv2d(dims[0], channels, 1)
    randomize_bn(m.eval())
    return {k: v.float() for k, v in m.state_dict().items() if v.dtype.is_floating_point}


class PairRunner(Runner):
    """test_hip_conv_blocks.Runner on images of any channel count"""

    def __init__(self, c, sd32, channels):
        super().__init__(c, sd32)
        g = torch.Generator().manual_seed(2000 + c.seed)
        self.x = torch.randn(c.B, channels, c.H, c.W, generator=g)
        self.x_dev = self.x.to(DEV)
        self.eps = torch.empty(self.rows, channels, c.H, c.W, dtype=torch.float32, device=DEV)

    def profiled_forward(self, value):
        self.ws.view(torch.float32).fill_(value)
        self.eps.fill_(value)
        _hip.profile_begin()
        status = self.forward()
        torch.cuda.synchronize()
        prof = _hip.profile_end()
        check(status, "dt_unet_forward")
        return {n: v["launches"] for n, v in prof.items()}


@pytest.fixture(scope="module")
def cpu_threads():
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(old, 16)))
    yield
    torch.set_num_threads(old)


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_pair_kernel_equals_the_256x64_kernel_and_float64(shape, monkeypatch, cpu_threads):
    name, channels, dims, H, W, B, n_pass, tb_div, seed, pins = shape
    c = Case(name, 0.0, H, W, B, n_pass, 0, tb_div, 0, seed)
    sd32 = custom_state_dict(channels, dims, seed)
    sd64 = {k: v.double() for k, v in sd32.items()}
    new = PairRunner(c, sd32, channels)
    monkeypatch.setenv("DT_NO_STRIP_PAIR", "1")          # read by dt_unet_create
    old = PairRunner(c, sd32, channels)
    monkeypatch.delenv("DT_NO_STRIP_PAIR")
    runs = {"pair": new, "256x64": old}

    # the heuristic plan's block outputs (no 256-row tile in it): the inputs of the float64 references, once per shape
    for run in runs.values():
        run.h.ensure_plan(run.rows, H, W, B, 0, tune=False)
        run.h.set_precision(_hip.PREC_AUTO)
    prof = new.profiled_forward(POISONS[0])
    assert PAIR not in prof and OLD not in prof, prof
    base = [new.act(j).clone() for j in range(8)]
    acts = [a[..., :cout].permute(0, 3, 1, 2).double().cpu() for a, cout in zip(base, new.couts)]
    refs = {j: (r.to(DEV), s.to(DEV)) for j, (r, s) in
            block_references(sd64, new.x.double()[new.imgs], acts, row_temb(sd32, new.conds, tb_div)).items()}

    failures = []
    for j, slot, splits, fuse, served in pins:
        what = f"{name} {BLOCK_NAMES[j]}.{SLOT_NAMES[slot]} 256x64 s{splits}{' +skip' if fuse else ''}"
        outs = {}
        for tag, run in runs.items():
            assert run.pin(j, slot, 256, 64, splits, STRIP32, fuse), what
            rep = run.report(j, slot)
            assert rep[:4] == (256, 64, splits, STRIP32 + 8 * fuse), f"{what}: resolves to {rep}"
            per_poison = []
            for value in POISONS:
                prof = run.profiled_forward(value)
                per_poison.append(([run.act(b).clone() for b in range(8)], run.eps.clone()))
            # the same choice is reported whichever kernel serves it; the profiler names the kernel
            expect = PAIR if (served and tag == "pair") else OLD
            other = OLD if expect == PAIR else PAIR
            print(f"{what} [{tag}]: report {rep}, 256-row launches {({n: k for n, k in prof.items() if '<256' in n})}")
            if prof.get(expect, 0) < 1 or other in prof:
                failures.append(f"{what} [{tag}]: expected {expect}, the profiler saw {prof}")
            for b in range(8):
                if not torch.equal(bits(per_poison[0][0][b]), bits(per_poison[1][0][b])):
                    failures.append(f"{what} [{tag}]: {BLOCK_NAMES[b]} differs between NaN- and 1e30-poisoned workspaces")
            if not torch.equal(bits(per_poison[0][1]), bits(per_poison[1][1])) or not torch.isfinite(per_poison[0][1]).all():
                failures.append(f"{what} [{tag}]: eps differs between poisons or is not finite")
            outs[tag] = per_poison[0]
            if slot == 2 and j == 0:
                # head fusion on (the default): enc1.conv2 stores the pool alone (skip_out); compared through enc2 and eps
                run.h.set_head_fusion(True)
                run.profiled_forward(POISONS[0])
                outs[tag] = (outs[tag][0] + [run.act(1).clone()], torch.cat([outs[tag][1], run.eps.clone()]))
                run.h.set_head_fusion(False)
        for b, (a_new, a_old) in enumerate(zip(outs["pair"][0], outs["256x64"][0])):
            if not torch.equal(bits(a_new), bits(a_old)):
                diff = (a_new.double() - a_old.double()).abs().max().item()
                where = BLOCK_NAMES[b] if b < 8 else "enc2 with head fusion on"
                failures.append(f"{what}: {where} differs between the two kernels (max {diff:.3e})")
        if not torch.equal(bits(outs["pair"][1]), bits(outs["256x64"][1])):
            failures.append(f"{what}: eps differs between the two kernels")
        for b in range(j):
            if not torch.equal(bits(outs["pair"][0][b]), bits(base[b])):
                failures.append(f"{what}: {BLOCK_NAMES[b]}, upstream of the pinned block, changed")
        ref, S = refs[j]
        bad, ratio, rel, pad, rms = check_block(outs["pair"][0][j], ref, S, new.couts[j]).tolist()
        print(f"{what}: max err/S {ratio * 2 ** 24:.3f} * 2^-24, per-image rel L2 {rel:.3e}, RMS err/S {rms * 2 ** 24:.4f} * 2^-24")
        if bad:
            failures.append(f"{what}: |err| > {C_TAU} * 2^-24 * S (max err/S = {ratio * 2 ** 24:.2f} * 2^-24)")
        if rel > REL_L2:
            failures.append(f"{what}: per-image relative L2 error {rel:.3e} > {REL_L2:.0e}")
        if rms * 2 ** 24 > RMS_C:
            failures.append(f"{what}: per-image RMS of err/S {rms * 2 ** 24:.3f} * 2^-24 > {RMS_C} * 2^-24")
        if pad:
            failures.append(f"{what}: nonzero padding channels")
    assert not failures, f"{len(failures)} failures:\n  " + "\n  ".join(failures[:40])
