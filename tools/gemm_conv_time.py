"""Times of the two tile-GEMM convolution kernels (conv_gemm_kernel, conv_gemm_bf16x6_kernel) where the default benchmark
config runs them, one line per cell.

The teacher (size factor 1.0) and the student (0.5) of bench.py's default config at its forward shape (2 x 256 rows of
16 x 16).  Per model and precision mode (auto, fp32): one warm forward on real noise, then every (block, slot) of
conv_choices() that resolves to the fp32 or the plain split-bf16 kind, timed at its resolved choice with
UNetHandle.time_conv (reps=50).  Then each of the eight kernels once on a full 3x3 layer of its natural size: pinned on the
teacher's enc2.conv2.

    python tools/gemm_conv_time.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from distillation_trajectories_amd import _hip, engine  # noqa: E402
from distillation_trajectories_amd._hip import COND_NONE, COND_ONE  # noqa: E402
from distillation_trajectories_amd.config import Config  # noqa: E402
from distillation_trajectories_amd.models import DiffusionUNet  # noqa: E402
from distillation_trajectories_amd.synthetic import make_model  # noqa: E402

DEV = "cuda:0"
REPS = 50
SLOTS = ("skip", "conv1", "conv2")
GEMM_KINDS = (_hip.KIND_FP32, 1)
TILES = ((128, 128), (128, 64), (64, 128), (64, 64))


def cell(name, timed):
    if timed is None:
        print(f"{name:64s} refused", flush=True)
    else:
        ms, flops = timed
        print(f"{name:64s} {ms * 1e3:9.2f} us  {flops / ms * 1e-9:7.1f} TF/s", flush=True)


def main():
    spec = bench.CONFIGS[1]
    H, B = spec["H"], spec["batch"]
    rows = 2 * B
    cfg = Config()
    cfg.image_size, cfg.timesteps, cfg.sample_steps = H, spec["T"], spec["T"]
    x = torch.randn(B, 3, H, H, generator=torch.Generator().manual_seed(1234)).to(DEV)
    teacher = None
    for sf in spec["sf"]:
        h = engine.UNetHandle(make_model(DiffusionUNet, cfg, sf).state_dict(), DEV)
        teacher = teacher or h
        tb = h.time_bias([spec["T"] - 1] * 2, [COND_NONE, COND_ONE])
        for mode, prec in (("auto", _hip.PREC_AUTO), ("fp32", _hip.PREC_FP32)):
            h.set_precision(prec)
            h.forward(x, tb, 2, B)
            torch.cuda.synchronize()
            for j, slot, bm, bn, sp, kind, fold, _ in list(h._choices(h.shape(rows, H, H))):
                if kind not in GEMM_KINDS:
                    continue
                name = (f"sf{sf} {mode} {engine.BLOCK_NAMES[j]}.{SLOTS[slot]} {_hip.KIND_NAMES[kind]}{'+skip' if fold else ''} "
                        f"{bm}x{bn} s{sp}")
                cell(name, h.time_conv(rows, H, H, j, slot, bm, bn, sp, kind, fold, reps=REPS))
    teacher.set_precision(_hip.PREC_AUTO)
    teacher.forward(x, teacher.time_bias([spec["T"] - 1] * 2, [COND_NONE, COND_ONE]), 2, B)
    torch.cuda.synchronize()
    for kind in GEMM_KINDS:
        for bm, bn in TILES:
            cell(f"sf{spec['sf'][0]} enc2.conv2 pinned {_hip.KIND_NAMES[kind]} {bm}x{bn} s1",
                 teacher.time_conv(rows, H, H, 1, 2, bm, bn, 1, kind, 0, reps=REPS))


if __name__ == "__main__":
    main()
