#!/usr/bin/env python3
"""Stage times of the device PCA (dt_pca_fit) for P teacher/student pairs, against sklearn's PCA on the host.

  shapes : 16 x 16 x 3 at T = 50 (n = 2 x 51 rows of E = 768) and the default Config, 32 x 32 x 3 at T = 100 (2 x 101 rows
           of E = 3072); P in {1, 64, 256} pairs of seeded random-walk trajectories, step-major on the device
  device : HIP events recorded inside dt_pca_fit at the stage boundaries -- mean + Gram, eigen (tridiagonalisation,
           bisection, inverse iteration, back-transformation), components + signs + scores; medians of --reps calls after
           one warm-up call, k = 2
  host   : sklearn PCA(n_components=2) as the reference calls it (default solver: randomized for these shapes) on the
           float32 rows of --host-pairs pairs (median per pair, after one warm-up call), with the host's thread count as it is (16 CPUs on the GPU boxes)

Prints one JSON line per case; --out also writes them to a file.

  python tools/pca_time.py [--reps 5] [--host-pairs 8] [--out profiles/pca_time.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

from distillation_trajectories_amd import engine   # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [("16x16x3_T50", 51, 768), ("32x32x3_T100", 101, 3072)]


def walk(seed, n, P, E):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(n, P, E, generator=g, device=DEV).cumsum(0) * 0.1 + 1.0).contiguous()


def device_case(n_each, E, P, reps):
    X, Y = walk(1, n_each, P, E), walk(2, n_each, P, E)
    stages = []
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        r = engine.device_pca(X, 2, Y, events=ev)
        torch.cuda.synchronize()
        if it:
            stages.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)] + [ev[0].elapsed_time(ev[3])])
    assert (r["status"] == 0).all()
    med = [statistics.median(s[i] for s in stages) for i in range(4)]
    return X, Y, dict(zip(("mean_gram_ms", "eigen_ms", "components_ms", "total_ms"), [round(m, 3) for m in med]))


def host_case(X, Y, pairs):
    try:
        from sklearn.decomposition import PCA
    except ImportError:
        return {"host_ms_per_pair": None, "host_note": "sklearn not installed"}
    times = []
    PCA(n_components=2).fit_transform(np.vstack([X[:, 0].cpu().numpy(), Y[:, 0].cpu().numpy()]))   # warm-up call
    for p in range(min(pairs, X.shape[1])):
        rows = np.vstack([X[:, p].cpu().numpy(), Y[:, p].cpu().numpy()])
        t0 = time.perf_counter()
        PCA(n_components=2).fit_transform(rows)
        times.append((time.perf_counter() - t0) * 1e3)
    return {"host_ms_per_pair": round(statistics.median(times), 3), "host_pairs": len(times),
            "host_threads": torch.get_num_threads()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name, n_each, E in SHAPES:
        runs = {P: device_case(n_each, E, P, args.reps) for P in (1, 64, 256)}
        host = host_case(runs[64][0], runs[64][1], args.host_pairs)
        for P, (_, _, dev) in runs.items():
            rec = {"shape": name, "n": 2 * n_each, "E": E, "P": P, "k": 2, **dev,
                   "device_ms_per_pair": round(dev["total_ms"] / P, 4), **host}
            if host["host_ms_per_pair"]:
                rec["host_over_device_per_pair"] = round(host["host_ms_per_pair"] / rec["device_ms_per_pair"], 1)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
