#!/usr/bin/env python3
"""Stage times of the feature-space Fréchet distance on the device (dt_fid_cov_distance) for P students against one shared
teacher set, against the host formula ``calculate_fid`` (np.cov + scipy sqrtm) on the same machine: before this route the
only thing that could score sets of more than 2048 rows.

  shapes : n samples per set in {2100, 10000, 50000} x P in {1, 11} problems, feature width D = 2048; seeded feature-like
           rows (a common offset per column, a decaying spectrum), the teacher set shared by all P problems
  device : HIP events recorded inside dt_fid_cov_distance at the stage boundaries -- means + traces, the two covariance
           products, the two Cholesky factorisations, N = L_a^T L_b and N N^T, the tridiagonalisation, bisection + sum;
           medians of --reps calls after one warm-up call.  The features are on the device already and the workspace
           allocation is outside the events.  covariance_tflops counts the fp64 flops of the tiles that are computed
           (two sets per problem, the teacher's anew for every problem).
           The covariance product exists in one form, on fp64 MFMA; the plain-FMA form it was timed against is in
           DESIGN 9r and is no longer in the library.
  host   : ``calculate_fid`` on the float32 rows of one problem: median of --host-reps calls after one warm-up call, with
           the host's thread count as it is; its cost does not depend on P, so a batch of P costs P times that
  check  : the device result of problem 0 against the host's, in units of s = tr S_a + tr S_b

Prints one JSON line per case; --out also writes them to a file.

  python tools/fid_cov_time.py [--reps 5] [--host-reps 3] [--out profiles/fid_cov_time.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch         # noqa: E402

from distillation_trajectories_amd import engine   # noqa: E402
from distillation_trajectories_amd.analysis.metrics.fid_score import calculate_fid   # noqa: E402

DEV = torch.device("cuda:0")
D = 2048
UPPER_TILES = (D // 64) * (D // 64 + 1) // 2      # the 64 x 64 tiles a covariance product computes (the rest are mirrored)
STAGES = ("means_ms", "covariances_ms", "cholesky_ms", "cross_square_ms", "tridiag_ms", "bisect_sum_ms", "total_ms")


def features(seed, P, n, shift):
    """[P, n, D] fp32 on the device: offset + spread * (coefficients with a 1/sqrt(1+j) spectrum) @ (a random basis),
    one problem at a time so that the float64 intermediate stays small"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    basis = torch.randn(D, D, generator=g, device=DEV, dtype=torch.float64) / D ** 0.5
    decay = torch.rsqrt(1.0 + torch.arange(D, device=DEV, dtype=torch.float64))
    base = 0.4 * (1.0 + torch.rand(D, generator=g, device=DEV, dtype=torch.float64)) + shift
    out = torch.empty(P, n, D, dtype=torch.float32, device=DEV)
    for p in range(P):
        coeff = torch.randn(n, D, generator=g, device=DEV, dtype=torch.float64) * decay
        out[p] = (base + 0.15 * (coeff @ basis)).float()
    return out


def device_case(teacher, students, reps):
    n_ev = engine.FID_COV_EVENTS
    rows = []
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_ev)]
        r = engine.device_fid_cov(teacher, students, events=ev)
        torch.cuda.synchronize()
        if it:
            rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(n_ev - 1)] + [ev[0].elapsed_time(ev[-1])])
    assert (r["status"] == 0).all()
    med = [statistics.median(row[i] for row in rows) for i in range(n_ev)]
    return r, dict(zip(STAGES, [round(m, 3) for m in med]))


def host_case(teacher, student, reps):
    a, b = teacher.cpu().numpy(), student.cpu().numpy()
    times = []
    for it in range(reps + 1):
        t0 = time.perf_counter()
        fid = calculate_fid(a, b)
        if it:
            times.append((time.perf_counter() - t0) * 1e3)
    return fid, round(statistics.median(times), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3, help="0: leave the host formula out")
    ap.add_argument("--sizes", type=int, nargs="*", default=[2100, 10000, 50000])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 11])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n in args.sizes:
        teacher = features(1, 1, n, 0.0)[0]
        host = None
        for P in args.batches:
            students = features(2, P, n, 0.01)
            r, dev = device_case(teacher, students, args.reps)
            s = float(r["parts"][0, 1] + r["parts"][0, 2])
            rec = {"n": n, "P": P, "D": D, **dev, "device_ms_per_problem": round(dev["total_ms"] / P, 3),
                   "covariance_tflops": round(2 * P * UPPER_TILES * 2 * 64 * 64 * n * 1e-9 / dev["covariances_ms"], 2)}
            if args.host_reps:
                if host is None:                   # the first batch: problem 0 is the same rows for every P
                    host = host_case(teacher, students[0], args.host_reps)
                rec.update({"host_ms_per_problem": host[1], "host_threads": torch.get_num_threads(),
                            "host_over_device_per_problem": round(host[1] * P / dev["total_ms"], 1),
                            "device_minus_host_over_s": float(f"{abs(float(r['fid'][0]) - host[0]) / s:.3g}")})
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del students, r
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
