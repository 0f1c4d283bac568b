"""conv2 + folded 1x1 skip walk (one launch) under explicit (arithmetic, tile) choices, 20 back-to-back launches each."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.config import Config
from distillation_trajectories_amd.models import DiffusionUNet
from distillation_trajectories_amd.synthetic import make_model
sf = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
cfg = Config(); cfg.image_size = 16
m = make_model(DiffusionUNet, cfg, sf).to("cuda:0")
h = engine.UNetHandle.for_module(m)
x = torch.randn(256, 3, 16, 16, device="cuda:0")
tb = h.time_bias([10, 10], [_hip.COND_NONE, _hip.COND_ONE])
h.forward(x, tb, 2, 256, tune=False)
LAYERS = ((1, "enc2.conv2"), (2, "enc3.conv2"), (5, "dec3.conv2"), (6, "dec2.conv2"), (7, "dec1.conv2"))
for rnd in range(2):
    for prec, bm, bn, fuse in ((4, 128, 128, 1), (4, 64, 128, 1), (4, 128, 64, 1), (4, 64, 64, 1), (4, 256, 64, 1), (5, 128, 64, 1), (5, 64, 64, 1),
                               (5, 64, 128, 1), (4, 64, 64, 0), (5, 64, 64, 0), (5, 128, 64, 0), (5, 64, 128, 0)):
        row = f"prec {prec} {bm:3d}x{bn:<3d} fuse {fuse}"
        for j, name in LAYERS:
            ms, fl = h.time_conv(512, 16, 16, j, 2, bm, bn, 1, prec, fuse, reps=20) or (0, 0)
            row += f" {name} {ms*1e3:6.1f}us ({fl/ms/1e9:4.0f})" if ms > 0 else f" {name}   n/a      "
        print(row, flush=True)
