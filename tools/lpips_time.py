"""Time LPIPS (v0.1, net='alex') on the device for 512 pairs at 32 x 32 and at 64 x 64: the feature pass (both image sets)
and the distance pass separately, and every layer on its own, next to the same restatement in fp32 on torch's own GPU ops
(tests/lpips_ref64.py with F.conv2d / max_pool2d on device tensors).  Random weights (timing does not depend on them).

    python tools/lpips_time.py [--pairs 512] [--warmup 3] [--reps 20]

Each figure is taken with device events around the launches of one call, after ``warmup`` untimed calls, over ``reps``
calls: median [min .. max] in microseconds.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lpips_ref64 as ref  # noqa: E402
from distillation_trajectories_amd import lpips  # noqa: E402
from distillation_trajectories_amd.evaluation.metrics import LPIPSModel  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return f"{t[0]:9.1f} us [{t[1]:8.1f} .. {t[2]:8.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = ref.random_state_dict(0, torch.float32)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    model = LPIPSModel(dev, weights=sd)
    h = model.handle
    n = args.pairs
    print(f"# {torch.cuda.get_device_name(dev)}, torch {torch.__version__}, fp32, {n} pairs, {args.warmup} warm-up calls, "
          f"median [min .. max] of {args.reps}")
    for H in (32, 64):
        a, b = ref.images(n, H, H, seed=H).to(dev), ref.images(n, H, H, seed=H + 1).to(dev)
        pa, pb = h.features(a), h.features(b)
        with torch.no_grad():
            ta, tb = ref.taps(sd_dev, a), ref.taps(sd_dev, b)

            def hip_features():
                h.features(a, out=pa)
                h.features(b, out=pb)

            def torch_features():
                ref.taps(sd_dev, a)
                ref.taps(sd_dev, b)

            print(f"{H}x{H} feature pass (2 x {n} images)  hip   {fmt(timed(hip_features, args.warmup, args.reps))}")
            print(f"{H}x{H} feature pass (2 x {n} images)  torch {fmt(timed(torch_features, args.warmup, args.reps))}")
            print(f"{H}x{H} distance pass ({n} pairs)       hip   "
                  f"{fmt(timed(lambda: h.distance(pa, pb, H, H), args.warmup, args.reps))}")
            print(f"{H}x{H} distance pass ({n} pairs)       torch "
                  f"{fmt(timed(lambda: ref.distance_from_taps(sd_dev, ta, tb), args.warmup, args.reps))}")
            x = ref.scale_input(sd_dev, a)
            x_hip = x.permute(0, 2, 3, 1).contiguous()
            for l in range(lpips.N_LAYERS):
                name, cin, cout, k, *_ = ref.LAYERS[l]
                y_hip = h.run_layers(x_hip, l, l + 1, H, H)
                t_hip = timed(lambda: h.run_layers(x_hip, l, l + 1, H, H), args.warmup, args.reps)
                t_torch = timed(lambda: ref.run_layer(sd_dev, l, x), args.warmup, args.reps)
                oh, ow = y_hip.shape[1:3]
                flop = 2.0 * n * oh * ow * cout * cin * k * k
                print(f"{H}x{H} layer {l} ({cin:3d}->{cout:3d} k{k:<2d} -> {oh}x{ow}, {n} images)  hip {fmt(t_hip)} "
                      f"{flop / t_hip[0] / 1e6:6.1f} TFLOP/s   torch {fmt(t_torch)} {flop / t_torch[0] / 1e6:6.1f} TFLOP/s")
                x = ref.run_layer(sd_dev, l, x)
                x_hip = y_hip
            d_hip = h.distance(pa, pb, H, H)
            d_torch = ref.distance_from_taps(sd_dev, ta, tb).sum(dim=1)
            print(f"# {H}x{H}: max relative difference hip vs torch fp32 over {n} pairs: "
                  f"{((d_hip - d_torch).abs() / d_torch).max().item():.2e}", flush=True)


if __name__ == "__main__":
    main()
