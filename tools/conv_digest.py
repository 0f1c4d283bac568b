"""SHA-256 of what the U-Net's convolution stack computes on seeded synthetic models.  Two builds that print the same lines
compute the same bits.

The cases are those of tests/test_hip_conv_blocks.py (size factors 1.0 / 0.5 / 0.3 / 0.4, 16 px with 41 images -- ragged
tiles down to M = 82 at 1x1 --, 32 px with 5 images, the mixed batch, the one-pass batch, and the rectangular pictures
16 x 48, 48 x 16, 16 x 112, 32 x 48 and 16 x 80), with its enumeration of the admissible (tile, split, fuse) pins.  Per case:

  * one line per (block, slot, kind in fp32 / split-bf16 / strip): the block output and eps of every admissible pin of that
    slot with that kind, folded into one hash in the sorted order of the pins (head fusion off);
  * one line per precision mode (auto, split-bf16, fp32): eps under the unpinned plan, head fusion on.

Then the fused small model (size factor 0.25 at 16 px): one forward and a 4-step `sample`.

    python tools/conv_digest.py
"""
import hashlib
import os
import sys
from collections import defaultdict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_hip_conv_blocks as blocks  # noqa: E402
from distillation_trajectories_amd import _hip, engine  # noqa: E402
from distillation_trajectories_amd._hip import COND_NONE, COND_ONE, RULE_PSAMPLE, check  # noqa: E402
from distillation_trajectories_amd.config import Config  # noqa: E402
from distillation_trajectories_amd.models import DiffusionUNet  # noqa: E402
from distillation_trajectories_amd.synthetic import make_model  # noqa: E402

DEV = blocks.DEV
KIND_GROUPS = {0: "fp32", 1: "split-bf16", 3: "strip", 4: "strip", 5: "strip"}
MODES = (("auto", _hip.PREC_AUTO), ("split-bf16", _hip.PREC_SPLIT_BF16), ("fp32", _hip.PREC_FP32))


def state_dict(sf):
    cfg = Config()
    cfg.image_size = 16
    return {k: v.float() for k, v in make_model(DiffusionUNet, cfg, sf).state_dict().items() if v.dtype.is_floating_point}


def fold(digest, t):
    digest.update(t.contiguous().cpu().numpy().tobytes())


def line(name, digest, n):
    print(f"{name:52s} {digest.hexdigest()}  {n}", flush=True)


def case_lines(c):
    run = blocks.Runner(c, state_dict(c.sf))
    h = run.h
    h.ensure_plan(run.rows, c.H, c.W, c.B, c.single, tune=False)
    found = run.admissible()
    groups = defaultdict(list)
    for key in sorted(found):
        groups[(key[0], key[1], KIND_GROUPS[key[5] & 7])].append(key)
    for (j, slot, kind), keys in sorted(groups.items()):
        digest, ran = hashlib.sha256(), 0
        for key in keys:
            assert run.pin(j, slot, *found[key]), key
            status = run.forward()
            if status < 0:
                continue          # refused at the launch (stripk's 64 x 64 tile on rows of more than 31 pixels)
            check(status, "dt_unet_forward")
            fold(digest, run.act(j))
            fold(digest, run.eps)
            ran += 1
        line(f"{c.name} {engine.BLOCK_NAMES[j]}.{blocks.SLOT_NAMES[slot]} {kind}", digest, f"{ran} pins")
    h.set_head_fusion(True)
    for name, mode in MODES:
        h.set_precision(mode)
        check(run.forward(), "dt_unet_forward")
        digest = hashlib.sha256()
        fold(digest, run.eps)
        line(f"{c.name} unpinned {name} eps", digest, f"finite {bool(torch.isfinite(run.eps).all())}")


def fused_lines():
    h = engine.UNetHandle(state_dict(0.25), DEV)
    assert h.fused_active(16, 16), h.dims
    B, E, n_steps = 7, 3 * 256, 4
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, 3, 16, 16, generator=g).to(DEV)
    eps = h.forward(x, h.time_bias([9, 9], [COND_NONE, COND_ONE]), 2, B)
    digest = hashlib.sha256()
    fold(digest, eps)
    line("fused sf0.25 16px B7 forward eps", digest, f"finite {bool(torch.isfinite(eps).all())}")
    ts = [30, 20, 10, 0]
    traj = torch.empty(n_steps + 1, B, E, device=DEV)
    traj[0] = torch.randn(B, E, generator=g).to(DEV)
    z = torch.randn(n_steps * B, E, generator=g).to(DEV)
    coef = [(0.99, 0.05, 0.02), (0.98, 0.04, 0.03), (0.985, 0.03, 0.01), (0.97, 0.06, 0.0)]
    tb = h.time_bias([t for t in ts for _ in (0, 1)], [COND_NONE, COND_ONE] * n_steps)
    h.sample(RULE_PSAMPLE, traj, 16, 16, tb, 2, coef, [t > 0 for t in ts], z=z, z_shift=[i * B for i in range(n_steps)], w_scalar=3.0)
    assert h.fused_active(16, 16)
    digest = hashlib.sha256()
    fold(digest, traj)
    line("fused sf0.25 16px B7 sample 4 steps", digest, f"finite {bool(torch.isfinite(traj).all())}")


def main():
    torch.set_num_threads(max(1, min(torch.get_num_threads(), 16)))
    for c in blocks.CASES:
        case_lines(c)
    fused_lines()


if __name__ == "__main__":
    main()
