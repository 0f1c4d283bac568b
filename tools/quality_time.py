#!/usr/bin/env python3
"""Stage times of the device sample-quality scores (dt_quality_scores: KID, precision / recall, density / coverage), against
the same numbers in float64 numpy on the same machine.

  shapes : (P = 11 students, n = 512 samples per set) against one shared teacher set, and (P = 1, n = 2048); feature width
           D = 2048, k = 5; seeded feature-like rows (a common offset per column, a decaying spectrum), teacher and students
           drawn from one pool so that the counts are mixed
  device : HIP events recorded inside dt_quality_scores at the stage boundaries -- the three Gram matrices, the radii, the
           counts, the kernel sums with KID and the outputs; medians of --reps calls after one warm-up call.  The features
           are on the device already and the workspace allocation is outside the events.
  host   : float64 numpy from the same definitions (Gram matrices by BLAS, radii by np.partition) on the float32 rows of
           one problem: median of --host-reps calls after one warm-up call, with the host's thread count as it is; its cost
           does not depend on P, so a batch of P costs P times that
  check  : the device counts of problem 0 equal the host's, and KID agrees to the printed difference

Prints one JSON line per case; --out also writes them to a file.

  python tools/quality_time.py [--reps 5] [--host-reps 3] [--out profiles/quality_time.txt]
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
D, K = 2048, 5
STAGES = ("gram_ms", "radii_ms", "counts_ms", "kid_ms", "total_ms")


def features(seed, P, n):
    """teacher [n, D] and students [P, n, D], fp32 on the device: one pool of offset + spread * (coefficients with a
    1/sqrt(1+j) spectrum) @ (a random basis), student p shifted by 0.002 p"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    basis = torch.randn(D, D, generator=g, device=DEV, dtype=torch.float64) / D ** 0.5
    coeff = torch.randn(P + 1, n, D, generator=g, device=DEV, dtype=torch.float64)
    coeff *= torch.rsqrt(1.0 + torch.arange(D, device=DEV, dtype=torch.float64))
    base = 0.4 * (1.0 + torch.rand(D, generator=g, device=DEV, dtype=torch.float64))
    rows = base + 0.15 * (coeff @ basis)
    rows[1:] += 0.002 * torch.arange(P, device=DEV, dtype=torch.float64)[:, None, None]
    rows = rows.float().contiguous()
    return rows[0], rows[1:]


def device_case(teacher, students, reps):
    rows = []
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(engine.QUALITY_EVENTS)]
        r = engine.device_quality(teacher, students, k=K, events=ev)
        torch.cuda.synchronize()
        if it:
            rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(4)] + [ev[0].elapsed_time(ev[4])])
    assert (r["status"] == 0).all()
    med = [statistics.median(row[i] for row in rows) for i in range(5)]
    return r, dict(zip(STAGES, [round(m, 3) for m in med]))


def host_quality(a, b, k):
    """(kid, counts) in float64 numpy"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    n_a, n_b = len(a), len(b)
    gaa, gbb, gab = a @ a.T, b @ b.T, a @ b.T
    da, db = np.diag(gaa), np.diag(gbb)
    daa = np.maximum(da[:, None] + da[None, :] - 2.0 * gaa, 0.0)
    dbb = np.maximum(db[:, None] + db[None, :] - 2.0 * gbb, 0.0)
    dab = np.maximum(da[:, None] + db[None, :] - 2.0 * gab, 0.0)
    np.fill_diagonal(daa, 0.0)
    np.fill_diagonal(dbb, 0.0)
    ra, rb = np.partition(daa, k, axis=1)[:, k], np.partition(dbb, k, axis=1)[:, k]
    in_a = dab < ra[:, None]
    counts = [int(in_a.any(axis=0).sum()), int((dab < rb[None, :]).any(axis=1).sum()), int(in_a.sum()),
              int((dab.min(axis=1) < ra).sum())]
    kaa, kbb, kab = ((g / D + 1.0) ** 3 for g in (gaa, gbb, gab))
    kid = ((kaa.sum() - np.trace(kaa)) / (n_a * (n_a - 1)) + (kbb.sum() - np.trace(kbb)) / (n_b * (n_b - 1))
           - 2.0 * kab.sum() / (n_a * n_b))
    return float(kid), counts


def host_case(teacher, student, reps):
    a, b = teacher.cpu().numpy(), student.cpu().numpy()
    times = []
    for it in range(reps + 1):
        t0 = time.perf_counter()
        res = host_quality(a, b, K)
        if it:
            times.append((time.perf_counter() - t0) * 1e3)
    return res, round(statistics.median(times), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--cases", type=int, nargs="*", default=[11, 512, 1, 2048], help="P n [P n ...]")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for P, n in zip(args.cases[::2], args.cases[1::2]):
        teacher, students = features(1, P, n)
        r, dev = device_case(teacher, students, args.reps)
        (kid, counts), host_ms = host_case(teacher, students[0], args.host_reps)
        rec = {"n": n, "P": P, "D": D, "k": K, **dev, "device_ms_per_problem": round(dev["total_ms"] / P, 4),
               "host_ms_per_problem": host_ms, "host_threads": torch.get_num_threads(),
               "host_over_device_per_problem": round(host_ms * P / dev["total_ms"], 1),
               "counts": r["counts"][0].tolist(), "counts_equal_host": r["counts"][0].tolist() == counts,
               "kid": float(r["kid"][0]), "device_minus_host_kid": float(f"{abs(float(r['kid'][0]) - kid):.3g}")}
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
