#!/usr/bin/env python3
"""Times of the device t-SNE (dt_tsne_affinities, dt_tsne_descend) for P teacher/student pairs, against sklearn on the host.

  shapes : (n, E) = (102, 768): 16 x 16 x 3 at T = 50; (202, 3072): the default Config, 32 x 32 x 3 at T = 100;
           (500, 768): the largest pair the analysis still embeds.  P in {1, 256} seeded random-walk pairs, step-major
  device : HIP events around engine.device_tsne, medians (and the range) of --reps calls after one warm-up call of the
           same shape.  affinities_ms is a call with max_iter = 0: the affinities and the closing KL pass of the descent
           kernel.  descend_ms_per_1000 is a call of 1000 iterations of the default schedule on given affinities, with
           the stop rules off (min_grad_norm 0, no progress limit) so that every problem runs them all.
  host   : one sklearn TSNE fit of one pair, method="exact" and the default method="barnes_hut" (what the reference
           calls), after a warm-up fit of a small problem, with the host's thread count as it is

Prints one JSON line per case; --out also writes them to a file.

  python tools/tsne_time.py [--reps 3] [--no-host] [--out profiles/tsne_time.txt]
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
SHAPES = [(102, 768), (202, 3072), (500, 768)]
ALL_ITERATIONS = dict(min_grad_norm=0.0, n_iter_without_progress=(10 ** 6, 10 ** 6))


def walk(seed, n, P, E):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(n, P, E, generator=g, device=DEV).cumsum(0) * 0.1 + 1.0).contiguous()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def summary(times):
    return {"median": round(statistics.median(times), 3), "min": round(min(times), 3), "max": round(max(times), 3)}


def device_case(n, E, P, reps):
    X, Y = walk(1, n // 2, P, E), walk(2, n - n // 2, P, E)
    perp = float(min(30, n // 5))
    y0 = 1e-4 * np.random.RandomState(42).standard_normal((n, 2)).astype(np.float32)
    aff = []
    for it in range(reps + 1):
        ms, r = timed(lambda: engine.device_tsne(X, Y, perplexity=perp, init=y0, max_iter=0, return_affinities=True))
        if it:
            aff.append(ms)
    assert (r["status"] == 0).all()
    runs = []
    for it in range(reps + 1):
        ms, out = timed(lambda: engine.device_tsne(X, Y, perplexity=perp, init=y0, max_iter=1000,
                                                   affinities=r["affinities"], **ALL_ITERATIONS))
        if it:
            runs.append(ms)
    assert (out["n_iter"] == 1000).all()
    rec = {"affinities_ms": summary(aff), "descend_ms_per_1000": summary(runs),
           "kl_median": round(float(out["kl_divergence"].median()), 5)}
    rows = np.vstack([X[:, 0].cpu().numpy(), Y[:, 0].cpu().numpy()])
    return rows, perp, y0, rec


def host_case(rows, perp, y0):
    try:
        from sklearn.manifold import TSNE
    except ImportError:
        return {"host_note": "sklearn not installed"}
    TSNE(perplexity=5.0, max_iter=250, init="random", random_state=0).fit(rows[:40])          # warm-up
    rec = {"host_threads": torch.get_num_threads()}
    for method in ("exact", "barnes_hut"):
        t0 = time.perf_counter()
        fit = TSNE(n_components=2, perplexity=perp, random_state=42, init=y0, method=method).fit(rows)
        rec[f"host_{method}_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec[f"host_{method}_kl"] = round(float(fit.kl_divergence_), 5)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n, E in SHAPES:
        host = None
        for P in (1, 256):
            rows, perp, y0, dev = device_case(n, E, P, args.reps)
            if host is None:
                host = {} if args.no_host else host_case(rows, perp, y0)
            total = dev["affinities_ms"]["median"] + dev["descend_ms_per_1000"]["median"]
            rec = {"n": n, "E": E, "P": P, "perplexity": perp, **dev, "device_ms_per_pair": round(total / P, 3), **host}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
