"""SHA-256 of what the two feature networks compute on seeded inputs and seeded random weights: every InceptionV3 module on
the device's own upstream output, the whole extractor, the LPIPS feature packs at every size of tests/lpips_ref64.py SIZES
and one distance.  Two builds that print the same lines compute the same bits.

    python tools/featnet_digest.py
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import inception_ref  # noqa: E402
import lpips_ref64  # noqa: E402
from distillation_trajectories_amd import inception  # noqa: E402
from distillation_trajectories_amd.analysis.metrics import fid_score  # noqa: E402
from distillation_trajectories_amd.evaluation.metrics import LPIPSModel  # noqa: E402


def line(name, t):
    t = t.contiguous().cpu()
    digest = hashlib.sha256(t.numpy().tobytes()).hexdigest()
    print(f"{name:28s} {digest}  nonzero {(t != 0).double().mean().item():.3f}", flush=True)


def main():
    dev = torch.device("cuda:0")
    sd = {k: v.float() for k, v in inception_ref.random_state_dict(inception.key_table(), seed=3).items()
          if v.is_floating_point()}
    model = fid_score.InceptionModel(dev, weights=sd)
    x = model.handle.preprocess(lpips_ref64.images(3, 32, 32, seed=4), 0.5, 0.5)
    for m, name in enumerate(inception.MODULES):
        x = model.handle.run_modules(x, m, m + 1)
        line(f"inception {name} B=3", x)
    line("inception features 24x40 B=5", fid_score.extract_features(lpips_ref64.images(5, 24, 40, seed=5), model))
    handle = LPIPSModel(dev, weights=lpips_ref64.random_state_dict(6, torch.float32)).handle
    for H, W in lpips_ref64.SIZES:
        a, b = (handle.features(lpips_ref64.images(5, H, W, seed=7 + H + i)) for i in range(2))
        line(f"lpips features {H}x{W} N=5", a)
        line(f"lpips distance {H}x{W} N=5", handle.distance(a, b, H, W))


if __name__ == "__main__":
    main()
