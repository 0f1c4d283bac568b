"""Time the device InceptionV3 feature extractor (fid_score.extract_features) for 100 and 1000 images of 32 x 32 against a
yardstick on the same GPU: the same network restated with torch F.conv2d in fp32 (MIOpen), BatchNorm unfolded, NCHW
(tests/inception_ref.py run on fp32 CUDA tensors).  Random weights (the timing does not depend on their values).

    python tools/fid_time.py [--batch 64] [--reps 3]

Prints one line per (path, N): median wall time of ``reps`` runs after one warm-up run, ms per image and TFLOP/s.
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import inception_ref as ref  # noqa: E402
from distillation_trajectories_amd import inception  # noqa: E402
from distillation_trajectories_amd.analysis.metrics import fid_score  # noqa: E402


def flops_per_image(sd):
    """2 * MACs of every convolution of one 299 x 299 forward, counted on the restatement."""
    total = [0]
    conv = F.conv2d

    def counting(x, w, *a, **k):
        y = conv(x, w, *a, **k)
        total[0] += 2 * y.numel() * w[0].numel()
        return y
    ref.F.conv2d = counting
    try:
        ref.features({k: v.double() for k, v in sd.items()}, torch.zeros(1, 3, 32, 32), 1.0, 0.0)
    finally:
        ref.F.conv2d = conv
    return total[0]


def torch_features(sd_dev, images, batch):
    mean = torch.tensor(ref.MEAN, device=images.device).view(1, 3, 1, 1)
    std = torch.tensor(ref.STD, device=images.device).view(1, 3, 1, 1)
    net, out = ref._Net(sd_dev), []
    with torch.no_grad():
        for i in range(0, len(images), batch):
            x = F.interpolate(images[i:i + batch], size=(299, 299), mode="bilinear", align_corners=False)
            x = (x - mean) / std
            for m in range(ref.N_MODULES):
                x = net.module(m, x)
            out.append(x)
    return torch.cat(out)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = {k: v.float() for k, v in ref.random_state_dict(inception.key_table(), seed=0).items() if v.is_floating_point()}
    flops = flops_per_image(sd)
    model = fid_score.InceptionModel(dev, weights=sd)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    print(f"# {torch.cuda.get_device_name(dev)}, torch {torch.__version__}, fp32, 32x32 inputs resized to 299x299, "
          f"batch {args.batch}, median of {args.reps} after 1 warm-up; {flops / 1e9:.2f} GFLOP per image")
    for n in (100, 1000):
        imgs = torch.tanh(torch.randn(n, 3, 32, 32, generator=torch.Generator().manual_seed(n))).to(dev)
        for name, fn in (("hip extract_features", lambda: fid_score.extract_features(imgs, model, batch_size=args.batch)),
                         ("torch F.conv2d (MIOpen)", lambda: torch_features(sd_dev, imgs, args.batch))):
            t = timed(fn, args.reps)
            print(f"{name:24s} N={n:5d}: {t * 1e3:9.1f} ms  {t * 1e3 / n:7.3f} ms/image  {flops * n / t / 1e12:6.1f} TFLOP/s",
                  flush=True)
    a = fid_score.extract_features(imgs[:64], model)
    b = torch_features(sd_dev, imgs[:64], args.batch)
    print(f"# max relative L2 difference hip vs torch fp32 over 64 images: "
          f"{((a - b).norm(dim=1) / b.norm(dim=1)).max().item():.2e}")


if __name__ == "__main__":
    main()
