#!/usr/bin/env python3
"""Times of the sliced Wasserstein distance (include/dt_hip_swd.h) on one MI355X.

The benchmark's own shape: 51 states (a 50-step trajectory), 256 samples per set, E = 768 (3 x 16 x 16), L = 512
directions, p = 2, one teacher against 4 students.  After --warmup calls, --reps calls bracketed by device events on the
stream and ended by a synchronise (the events' own clock; the board's clocks are neither set nor read: they are what the
machine runs at under this load); median, min and max are printed:

  sweep         what sliced_wasserstein_sweep does per guidance scale: engine.device_swd_sorted of the teacher once, then
                engine.device_swd(sorted teacher, student) for each of the students
  pair          engine.device_swd(teacher, student) for one student: both sets projected and sorted in one call; with it the
                fp64 rate of the two projections (a fused multiply-add counted as 2 FLOP) over the whole call and its share
                of the datasheet's vector fp64 peak (78.6 TFLOP/s)
  kernels       the in-library profiler's split of one `sweep` by kernel class (its own events around every launch)
  numpy_16      the same computation in numpy float64 on the host, the states spread over 16 threads: the teacher's
                projections made once, X @ theta^T, np.sort, mean((a - b)^2).  The time yardstick; its values are also
                compared with the stage's (largest relative difference of mean_w)

Prints one JSON line per row; --out also appends them to a file.

  python tools/swd_time.py [--reps 10] [--warmup 2] [--out profiles/swd_time.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--states", type=int, default=51)
ap.add_argument("--samples", type=int, default=256)
ap.add_argument("--width", type=int, default=768)
ap.add_argument("--directions", type=int, default=512)
ap.add_argument("--students", type=int, default=4)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

from distillation_trajectories_amd import _hip, engine   # noqa: E402

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


def main():
    from concurrent.futures import ThreadPoolExecutor
    dev = torch.device("cuda:0")
    n, S, E, L, K = args.states, args.samples, args.width, args.directions, args.students
    g = torch.Generator(device="cpu").manual_seed(1)
    X = torch.randn(n, S, E, generator=g).to(dev)
    Ys = [(X + 0.1 * (k + 1) * torch.randn(n, S, E, generator=g).to(dev)).contiguous() for k in range(K)]
    theta = engine.swd_directions(E, L).to(dev)
    shape = dict(states=n, samples=S, E=E, L=L, p=2, students=K, reps=args.reps, warmup=args.warmup)

    def sweep():
        made = engine.device_swd_sorted(X, theta)
        return [engine.device_swd(made, Y, p=2) for Y in Ys]

    t = timed(sweep)
    emit(what="sweep", **shape, **t)
    tp = timed(lambda: engine.device_swd(X, Ys[0], directions=theta, p=2))
    flops = 2.0 * 2 * n * S * E * L
    rate = flops / (tp["median_ms"] * 1e-3)
    emit(what="pair", **shape, **tp, projection_fp64_tflops=round(rate / 1e12, 2),
         share_of_vector_fp64_peak=round(rate / FP64_VECTOR_PEAK, 3))

    torch.cuda.synchronize()
    _hip.profile_begin()
    got = sweep()
    torch.cuda.synchronize()
    split = _hip.profile_end()
    emit(what="kernels", **{name: dict(launches=v["launches"], ms=round(v["ms"], 4)) for name, v in split.items()})
    assert not any(r["status"].any().item() for r in got)

    xh, yh, th = X.cpu().numpy(), [Y.cpu().numpy() for Y in Ys], theta.cpu().numpy().astype(np.float64)

    def state(i):
        a = np.sort(xh[i].astype(np.float64) @ th.T, axis=0)
        return [((a - np.sort(y[i].astype(np.float64) @ th.T, axis=0)) ** 2).mean() for y in yh]

    with ThreadPoolExecutor(max_workers=16) as pool:
        def once():
            t0 = time.perf_counter()
            res = list(pool.map(state, range(n)))
            return (time.perf_counter() - t0) * 1e3, np.array(res)
        once()
        runs = [once() for _ in range(3)]
    host_ms = statistics.median(r[0] for r in runs)
    want = runs[0][1]                                                     # [states, students]
    mine = np.stack([r["mean_w"].cpu().numpy() for r in got], axis=1)
    emit(what="numpy_16", threads=16, median_ms=round(host_ms, 1), hand_written_over_numpy=round(t["median_ms"] / host_ms, 5),
         largest_relative_difference_of_mean_w=float(f"{(np.abs(mine - want) / want).max():.3g}"))


if not torch.cuda.is_available():
    sys.exit("swd_time.py measures on the GPU; none is visible")
main()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
