#!/usr/bin/env python3
"""Times of the Sinkhorn divergence (include/dt_hip_sinkhorn.h) on one MI355X.

The benchmark's own shape: 51 states (a 50-step trajectory), 256 samples per set, E = 768 (3 x 16 x 16), p = 2, one teacher
against 4 students, rel_epsilon = 0.05, tol = 1e-9, max_iter as the engine's default.  After --warmup calls, --reps calls
bracketed by device events on the stream and ended by a synchronise (the events' own clock; the board's clocks are neither
set nor read: they are what the machine runs at under this load); median, min and max are printed:

  sweep         what sinkhorn_sweep does per guidance scale: the teacher's mean self cost and epsilon on the device, the
                teacher's self term once, then per student the cross term and the student's self term
                (engine.device_sinkhorn_divergence with the teacher's self term handed in)
  term          one engine.device_sinkhorn_ot(teacher, student): the cost matrices and the steps of 51 problems; with it the
                steps that were run and enqueued
  paired        the same sweep for students that follow the teacher sample by sample (teacher + 0.1 (k + 1) noise), which is
                what the sweep's ``divergence`` compares: the cross terms never reach tol = 1e-9 (see main) and run all
                max_iter steps; and once more at the engine's default tol
  kernels       the in-library profiler's split of one `sweep` by kernel class (its own events around every launch)
  numpy_16      the same computation in numpy float64 on the host, the states spread over 16 threads: cost matrices from the
                Gram expansion |a|^2 + |b|^2 - 2 a.b (a matrix product; the stage itself forms differences), the same
                log-domain steps and stopping rule.  The time yardstick; its values are also compared with the stage's
                (largest relative difference of the divergence)

Prints one JSON line per row; --out also appends them to a file.

  python tools/sinkhorn_time.py [--reps 5] [--warmup 1] [--out profiles/sinkhorn_time.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--states", type=int, default=51)
ap.add_argument("--samples", type=int, default=256)
ap.add_argument("--width", type=int, default=768)
ap.add_argument("--students", type=int, default=4)
ap.add_argument("--rel-epsilon", type=float, default=0.05)
ap.add_argument("--tol", type=float, default=1e-9)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

from distillation_trajectories_amd import _hip, engine   # noqa: E402

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


def host_ot(C, eps, max_iter, tol):
    g = np.zeros(C.shape[1])
    logn_a, logn_b = np.log(C.shape[0]), np.log(C.shape[1])
    for _ in range(max_iter):
        z = (g[None, :] - C) / eps
        m = z.max(axis=1)
        f = -eps * (m + np.log(np.exp(z - m[:, None]).sum(axis=1)) - logn_b)
        z = (f[:, None] - C) / eps
        m = z.max(axis=0)
        gn = -eps * (m + np.log(np.exp(z - m[None, :]).sum(axis=0)) - logn_a)
        err = np.abs(np.expm1((g - gn) / eps)).mean()
        g = gn
        if err <= tol:
            break
    return f.mean() + g.mean()


def host_cost(a, b):
    c = (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] - 2.0 * (a @ b.T)
    return np.maximum(c, 0.0)


def main():
    from concurrent.futures import ThreadPoolExecutor
    dev = torch.device("cuda:0")
    n, S, E, K = args.states, args.samples, args.width, args.students
    max_iter, tol, rel = engine.SINKHORN_DEFAULT_MAX_ITER, args.tol, args.rel_epsilon
    g = torch.Generator(device="cpu").manual_seed(1)
    X = torch.randn(n, S, E, generator=g).to(dev)
    # students as draws of their own, a little wider than the teacher's: a student within a fraction of epsilon of the
    # teacher sample by sample makes the plan a near-permutation whose per-sample gauges are coupled by exp(-gap / eps) only,
    # and err then stays near n exp(-gap / eps) (5e-8 at X + 0.1 noise) for millions of steps: tol = 1e-9 is out of reach there
    Ys = [((1.0 + 0.05 * (k + 1)) * torch.randn(n, S, E, generator=g)).to(dev) for k in range(K)]
    shape = dict(states=n, samples=S, E=E, p=2, students=K, rel_epsilon=rel, tol=tol, max_iter=max_iter, reps=args.reps,
                 warmup=args.warmup)

    def sweep():
        eps = engine.device_sinkhorn_mean_cost(X, X)["mean_cost"] * rel
        own = engine.device_sinkhorn_ot(X, X, eps, max_iter=max_iter, tol=tol)
        return [engine.device_sinkhorn_divergence(X, Y, eps, max_iter=max_iter, tol=tol, self_a=own) for Y in Ys]

    t = timed(sweep)
    emit(what="sweep", **shape, **t)
    eps = engine.device_sinkhorn_mean_cost(X, X)["mean_cost"] * rel
    tt = timed(lambda: engine.device_sinkhorn_ot(X, Ys[0], eps, max_iter=max_iter, tol=tol))
    one = engine.device_sinkhorn_ot(X, Ys[0], eps, max_iter=max_iter, tol=tol)
    emit(what="term", **shape, **tt, steps_run_max=int(one["iters"].max().item()), steps_enqueued=max_iter,
         launches=2 * max_iter + 5)

    Yp = [(X + 0.1 * (k + 1) * torch.randn(n, S, E, generator=g).to(dev)).contiguous() for k in range(K)]

    def paired(tolerance):
        e = engine.device_sinkhorn_mean_cost(X, X)["mean_cost"] * rel
        own = engine.device_sinkhorn_ot(X, X, e, max_iter=max_iter, tol=tolerance)
        return [engine.device_sinkhorn_divergence(X, Y, e, max_iter=max_iter, tol=tolerance, self_a=own) for Y in Yp]

    for tolerance in (tol, engine.SINKHORN_DEFAULT_TOL):
        tp = timed(lambda: paired(tolerance))
        res = paired(tolerance)
        emit(what="paired", **dict(shape, tol=tolerance), **tp, steps_max=[int(r["iters"].max().item()) for r in res],
             not_converged=[int((r["status"] & 4).ne(0).sum().item()) for r in res],
             err_max=[float(f"{r['err'].max().item():.3g}") for r in res])

    torch.cuda.synchronize()
    _hip.profile_begin()
    got = sweep()
    torch.cuda.synchronize()
    split = _hip.profile_end()
    emit(what="kernels", **{name: dict(launches=v["launches"], ms=round(v["ms"], 4)) for name, v in split.items()})
    assert not any((r["status"] & 3).any().item() for r in got)
    emit(what="convergence", steps_max=[int(r["iters"].max().item()) for r in got],
         not_converged=[int((r["status"] & 4).ne(0).sum().item()) for r in got], err_max=[float(f"{r['err'].max().item():.3g}") for r in got])

    xh, yh = X.cpu().numpy().astype(np.float64), [Y.cpu().numpy().astype(np.float64) for Y in Ys]

    def state(i):
        caa = host_cost(xh[i], xh[i])
        e = rel * caa.mean()
        aa = host_ot(caa, e, max_iter, tol)
        return [host_ot(host_cost(xh[i], y[i]), e, max_iter, tol) - (0.5 * aa + 0.5 * host_ot(host_cost(y[i], y[i]), e, max_iter, tol))
                for y in yh]

    with ThreadPoolExecutor(max_workers=16) as pool:
        def once():
            t0 = time.perf_counter()
            res = list(pool.map(state, range(n)))
            return (time.perf_counter() - t0) * 1e3, np.array(res)
        runs = [once() for _ in range(2)]
    host_ms = min(r[0] for r in runs)
    want = runs[0][1]                                                     # [states, students]
    mine = np.stack([r["divergence"].cpu().numpy() for r in got], axis=1)
    emit(what="numpy_16", threads=16, best_ms=round(host_ms, 1), hand_written_over_numpy=round(t["median_ms"] / host_ms, 5),
         largest_relative_difference_of_divergence=float(f"{(np.abs(mine - want) / np.abs(want)).max():.3g}"))


if not torch.cuda.is_available():
    sys.exit("sinkhorn_time.py measures on the GPU; none is visible")
main()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
