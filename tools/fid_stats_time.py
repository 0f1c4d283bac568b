#!/usr/bin/env python3
"""Stage times of the device Fréchet distance (dt_fid_distance) for P students against one shared teacher set, against the
host formula ``calculate_fid`` (np.cov + scipy sqrtm, the default path of the FID drivers) on the same machine.

  shapes : n samples per set in {50, 500, 2048} x P in {1, 11, 44} problems, feature width D = 2048; seeded feature-like
           rows (a common offset per column, a decaying spectrum), the teacher set shared by all P problems
  device : HIP events recorded inside dt_fid_distance at the stage boundaries -- means + traces, the two products
           (M = A_c B_c^T, then M M^T), the tridiagonalisation, bisection + sum; medians of --reps calls after one warm-up
           call.  The features are on the device already and the workspace allocation is outside the events.
  host   : ``calculate_fid`` on the float32 rows of one problem: median of --host-reps calls after one warm-up call, with
           the host's thread count as it is; its cost does not depend on P, so a batch of P costs P times that
  check  : the device result of problem 0 against the host's, in units of s = tr S_a + tr S_b

Prints one JSON line per case; --out also writes them to a file.

  python tools/fid_stats_time.py [--reps 5] [--host-reps 3] [--out profiles/fid_stats_time.txt]
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
STAGES = ("means_ms", "products_ms", "tridiag_ms", "bisect_sum_ms", "total_ms")


def features(seed, P, n, shift):
    """[P, n, D] fp32 on the device: offset + spread * (coefficients with a 1/sqrt(1+j) spectrum) @ (a random basis)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    basis = torch.randn(D, D, generator=g, device=DEV, dtype=torch.float64) / D ** 0.5
    coeff = torch.randn(P, n, D, generator=g, device=DEV, dtype=torch.float64)
    coeff *= torch.rsqrt(1.0 + torch.arange(D, device=DEV, dtype=torch.float64))
    base = 0.4 * (1.0 + torch.rand(D, generator=g, device=DEV, dtype=torch.float64)) + shift
    return (base + 0.15 * (coeff @ basis)).float().contiguous()


def device_case(teacher, students, reps):
    rows = []
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(engine.FID_EVENTS)]
        r = engine.device_fid(teacher, students, events=ev)
        torch.cuda.synchronize()
        if it:
            rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(4)] + [ev[0].elapsed_time(ev[4])])
    assert (r["status"] == 0).all()
    med = [statistics.median(row[i] for row in rows) for i in range(5)]
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
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[50, 500, 2048])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 11, 44])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n in args.sizes:
        teacher = features(1, 1, n, 0.0)[0]
        host = None
        for P in args.batches:
            students = features(2, P, n, 0.01)
            r, dev = device_case(teacher, students, args.reps)
            if host is None:                       # P = 1 comes first: the host sees the rows the device just had
                host = host_case(teacher, features(2, 1, n, 0.01)[0], args.host_reps)
            s = float(r["parts"][0, 1] + r["parts"][0, 2])
            rec = {"n": n, "P": P, "D": D, **dev, "device_ms_per_problem": round(dev["total_ms"] / P, 4),
                   "host_ms_per_problem": host[1], "host_threads": torch.get_num_threads(),
                   "host_over_device_per_problem": round(host[1] * P / dev["total_ms"], 1)}
            if P == 1:
                rec["device_minus_host_over_s"] = float(f"{abs(float(r['fid'][0]) - host[0]) / s:.3g}")
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
