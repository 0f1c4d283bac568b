#!/usr/bin/env python3
"""Stage times of the row-panel route of the device sample-quality scores (dt_quality_stream_scores: KID, precision /
recall, density / coverage for sets of more than 2048 rows), beside the whole-matrix route at the one shape both take and
beside float64 numpy on the same machine.

  shapes : feature width D = 2048, k = 5; seeded feature-like rows (a common offset per column, a decaying spectrum),
           teacher and students drawn from one pool so that the counts are mixed.
             P = 1,  n = 2048            beside engine.device_quality (the only like-for-like comparison: the panel
                                         route forms all of A x A and B x B, 1.5 times the tile work)
             P = 1,  n = 10 000, 50 000
             P = 11, n = 10 000          the teacher shared (its side formed once), and the teacher copied 11 times
  device : HIP events recorded inside the entry point at the stage boundaries -- the diagonals and flags, the A side
           (Gram panels, radii, kernel sums), the B side, the A x B panels (Gram panels, counts, kernel sums), the
           finish; medians of --reps calls after one warm-up call.  The features are on the device already and the
           workspace allocation is outside the events.
  host   : at n = 10 000, one problem in float64 numpy from the same definitions, in row blocks of 1000 (no n x n
           matrix either), with the host's thread count as it is: one run.  Its counts must equal the device's.

Prints one JSON line per case; --out also writes them to a file.

  python tools/quality_stream_time.py [--reps 5] [--out profiles/quality_stream_time.txt]
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
STAGES = ("diag_ms", "a_side_ms", "b_side_ms", "cross_ms", "finish_ms", "total_ms")
OLD_STAGES = ("gram_ms", "radii_ms", "counts_ms", "kid_ms", "total_ms")


def features(seed, P, n):
    """teacher [n, D] and students [P, n, D], fp32 on the device: one pool of offset + spread * (coefficients with a
    1/sqrt(1+j) spectrum) @ (a random basis), student p shifted by 0.002 p; made set by set, so that the float64
    intermediates stay small"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    basis = torch.randn(D, D, generator=g, device=DEV, dtype=torch.float64) / D ** 0.5
    base = 0.4 * (1.0 + torch.rand(D, generator=g, device=DEV, dtype=torch.float64))
    scale = torch.rsqrt(1.0 + torch.arange(D, device=DEV, dtype=torch.float64))
    sets = []
    for p in range(P + 1):
        coeff = torch.randn(n, D, generator=g, device=DEV, dtype=torch.float64) * scale
        sets.append((base + 0.15 * (coeff @ basis) + (0.002 * (p - 1) if p else 0.0)).float())
    return sets[0].contiguous(), torch.stack(sets[1:]).contiguous()


def timed(call, n_events, reps):
    rows = []
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_events)]
        r = call(ev)
        torch.cuda.synchronize()
        if it:
            rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(n_events - 1)] + [ev[0].elapsed_time(ev[-1])])
    assert (r["status"] == 0).all()
    return r, [round(statistics.median(row[i] for row in rows), 3) for i in range(n_events)]


def host_quality(a, b, k, block=1000):
    """(kid, counts) in float64 numpy, in row blocks: the definitions of include/dt_hip_quality.h without an n x n matrix"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    n_a, n_b = len(a), len(b)
    da, db = (a * a).sum(axis=1), (b * b).sum(axis=1)

    def side(x, dx):
        r2, s = np.empty(len(x)), 0.0
        for r0 in range(0, len(x), block):
            g = x[r0:r0 + block] @ x.T
            d = np.maximum(dx[r0:r0 + block, None] + dx[None, :] - 2.0 * g, 0.0)
            rows = np.arange(len(g))
            d[rows, r0 + rows] = 0.0
            r2[r0:r0 + block] = np.partition(d, k, axis=1)[:, k]
            kap = (g / D + 1.0) ** 3
            s += kap.sum() - kap[rows, r0 + rows].sum()
        return r2, s

    (ra, saa), (rb, sbb) = side(a, da), side(b, db)
    precision, recall, density, coverage, sab = np.zeros(n_b, bool), 0, 0, 0, 0.0
    for r0 in range(0, n_a, block):
        g = a[r0:r0 + block] @ b.T
        d = np.maximum(da[r0:r0 + block, None] + db[None, :] - 2.0 * g, 0.0)
        in_a = d < ra[r0:r0 + block, None]
        precision |= in_a.any(axis=0)
        recall += int((d < rb[None, :]).any(axis=1).sum())
        density += int(in_a.sum())
        coverage += int(in_a.any(axis=1).sum())
        sab += ((g / D + 1.0) ** 3).sum()
    kid = saa / (n_a * (n_a - 1)) + sbb / (n_b * (n_b - 1)) - 2.0 * sab / (n_a * n_b)
    return float(kid), [int(precision.sum()), recall, density, coverage]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=["1x2048", "1x10000", "1x50000", "11x10000"], help="PxN ...")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for case in args.cases:
        P, n = (int(v) for v in case.split("x"))
        teacher, students = features(1, P, n)
        rows = engine.quality_stream_panel_rows(engine._hip.load(), P, n, n, D)
        r, med = timed(lambda ev: engine.device_quality_stream(teacher, students, k=K, events=ev),
                       engine.QUALITY_STREAM_EVENTS, args.reps)
        rec = {"route": "panels", "teacher": "shared" if P > 1 else "one problem", "n": n, "P": P, "D": D, "k": K,
               "panel_rows": rows, **dict(zip(STAGES, med)), "ms_per_problem": round(med[-1] / P, 3),
               "counts": r["counts"][0].tolist(), "kid": float(r["kid"][0])}
        emit(rec)
        if n <= engine.QUALITY_MAX_ROWS:
            old, med_old = timed(lambda ev: engine.device_quality(teacher, students, k=K, events=ev), engine.QUALITY_EVENTS,
                                 args.reps)
            emit({"route": "matrices", "n": n, "P": P, "D": D, "k": K, **dict(zip(OLD_STAGES, med_old)),
                  "panels_over_matrices": round(med[-1] / med_old[-1], 2),
                  "counts_equal_panels": old["counts"].tolist() == r["counts"].tolist(),
                  "kid_minus_panels": float(f"{abs(float(old['kid'][0]) - float(r['kid'][0])):.3g}")})
            del old
        if P > 1:
            copied = teacher.unsqueeze(0).repeat(P, 1, 1)
            rc, med_c = timed(lambda ev: engine.device_quality_stream(copied, students, k=K, events=ev),
                              engine.QUALITY_STREAM_EVENTS, args.reps)
            emit({"route": "panels", "teacher": "copied", "n": n, "P": P, "D": D, "k": K, "panel_rows": rows,
                  **dict(zip(STAGES, med_c)), "ms_per_problem": round(med_c[-1] / P, 3),
                  "copied_over_shared": round(med_c[-1] / med[-1], 3),
                  "bits_equal_shared": all(rc[f].cpu().numpy().tobytes() == r[f].cpu().numpy().tobytes()
                                           for f in ("kid", "counts"))})
            del copied, rc
        if n == 10000 and P == 1 and not args.no_host:
            t0 = time.perf_counter()
            kid, counts = host_quality(teacher.cpu().numpy(), students[0].cpu().numpy(), K)
            host_ms = (time.perf_counter() - t0) * 1e3
            emit({"route": "host numpy float64, row blocks of 1000", "n": n, "P": 1, "D": D, "k": K,
                  "host_ms": round(host_ms, 1), "host_threads": torch.get_num_threads(),
                  "host_over_device": round(host_ms / med[-1], 1), "counts": counts,
                  "counts_equal_device": counts == r["counts"][0].tolist(),
                  "device_minus_host_kid": float(f"{abs(float(r['kid'][0]) - kid):.3g}")})
        del teacher, students, r
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
