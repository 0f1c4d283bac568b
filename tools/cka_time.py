#!/usr/bin/env python3
"""Times of layer-wise CKA (include/dt_hip_cka.h) on one MI355X.

Two shapes: (a) the teacher (size factor 1.0) against a size-factor 0.5 student at 16 x 16 on n = 256 states, a typical
sweep cell, and (b) the same pair at 32 x 32 on n = 1024.  For each, after --warmup calls, --reps calls bracketed by device
events on the stream and ended by a synchronise (the events' own clock; the board's clocks are neither set nor read: they
are what the machine runs at under this load); median, min and max are printed:

  readout       UNetHandle.block_features of one model: a forward on the layered kernels with the head launched separately
  gram          engine.device_cka_gram of the teacher's eight block outputs, read in place from the forward's workspace;
                with it the fp64 rate (n^2 p FLOP per layer: the upper triangle of n x n cells, a fused multiply-add per
                cell and feature) and its share of the datasheet's vector fp64 peak (78.6 TFLOP/s)
  scores        engine.device_cka of the teacher's Grams against the student's: 64 pairs
  end_to_end    both readouts, both Gram calls, the scores
  torch_gram    the same eight Grams by torch in float64 on the device: strip the pad channels, cast, subtract the column
                means, X @ X.T.  The time yardstick only; its values are not used anywhere.

Prints one JSON line per row; --out also appends them to a file.

  python tools/cka_time.py [--reps 10] [--warmup 2] [--cases a,b] [--out profiles/cka_time.txt]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--cases", default="a,b")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch         # noqa: E402

from distillation_trajectories_amd import engine   # noqa: E402
from distillation_trajectories_amd._hip import COND_ONE   # noqa: E402
from distillation_trajectories_amd.config import Config   # noqa: E402
from distillation_trajectories_amd.models import DiffusionUNet   # noqa: E402
from distillation_trajectories_amd.synthetic import make_model, seeded_noise   # noqa: E402

CASES = {"a": dict(H=16, n=256), "b": dict(H=32, n=1024)}
FP64_VECTOR_PEAK = 78.6e12          # MI355X datasheet, vector fp64
LINES = []


def emit(**row):
    line = json.dumps(row)
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def torch_grams(feats):
    out = []
    for f in feats:
        X = f.dense().double()
        X -= X.mean(dim=0, keepdim=True)
        out.append(X @ X.T)
    return out


def run_case(name, H, n):
    dev = torch.device("cuda:0")
    cfg = Config()
    cfg.image_size = H
    teacher = make_model(DiffusionUNet, cfg, 1.0).to(dev).eval()
    student = make_model(DiffusionUNet, cfg, 0.5).to(dev).eval()
    ht, hs = engine.UNetHandle.for_module(teacher), engine.UNetHandle.for_module(student)
    x = seeded_noise(3, (n, cfg.channels, H, H)).to(dev)
    tbt, tbs = ht.time_bias([25], [COND_ONE]), hs.time_bias([25], [COND_ONE])
    shape = dict(case=name, n=n, H=H, teacher_dims=ht.dims, student_dims=hs.dims, reps=args.reps, warmup=args.warmup)

    emit(what="readout", model="teacher", **shape, **timed(lambda: ht.block_features(x, tbt, 1, n)))
    emit(what="readout", model="student", **shape, **timed(lambda: hs.block_features(x, tbs, 1, n)))
    ft, fs = ht.block_features(x, tbt, 1, n), hs.block_features(x, tbs, 1, n)
    widths = [f.view.shape[1] * f.view.shape[2] * f.c for f in ft]
    t = timed(lambda: engine.device_cka_gram(ft))
    flops = float(n) * n * sum(widths)
    rate = flops / (t["median_ms"] * 1e-3)
    emit(what="gram", side="teacher", **shape, **t, features=widths, fp64_tflops=round(rate / 1e12, 2),
         share_of_vector_fp64_peak=round(rate / FP64_VECTOR_PEAK, 3), input_bytes=4 * n * sum(f.view.shape[1] * f.view.shape[2] * f.view.shape[3] for f in ft))
    tt = timed(lambda: torch_grams(ft))
    emit(what="torch_gram", side="teacher", **shape, **tt, hand_written_over_torch=round(t["median_ms"] / tt["median_ms"], 3))
    gt, gs = engine.device_cka_gram(ft), engine.device_cka_gram(fs)
    emit(what="scores", pairs=64, **shape, **timed(lambda: engine.device_cka(gt, gs)))

    def whole():
        a = engine.device_cka_gram(ht.block_features(x, tbt, 1, n))
        b = engine.device_cka_gram(hs.block_features(x, tbs, 1, n))
        return engine.device_cka(a, b)

    emit(what="end_to_end", **shape, **timed(whole))
    r = whole()
    assert not r["status_a"].any().item() and not r["status_b"].any().item()
    emit(what="values", case=name, cka_diagonal=[round(v, 4) for v in torch.diagonal(r["cka"]).tolist()],
         cka_unbiased_diagonal=[round(v, 4) for v in torch.diagonal(r["cka_unbiased"]).tolist()])


if not torch.cuda.is_available():
    sys.exit("cka_time.py measures on the GPU; none is visible")
for c in args.cases.split(","):
    run_case(c, **CASES[c])
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
