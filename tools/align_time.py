#!/usr/bin/env python3
"""Times of trajectory alignment (include/dt_hip_align.h) on one MI355X.

Two shapes: (a) 256 pairs of 51 x 51 states at E = 768, the benchmark's own trajectories, and (b) 64 pairs of 1001 x 1001 at
E = 3072 (configs[4]).  For each, on preallocated buffers, after --warmup calls, --reps calls bracketed by device events on
the stream and ended by a synchronise; median, min and max are printed:

  cost          dt_align_cost alone; with it the fp64 rate 3 P n_a n_b E / time (a subtraction and a fused multiply-add per
                element and cell) and its share of the datasheet's vector fp64 peak (78.6 TFLOP/s)
  dp            dt_align_dp alone on that matrix, per kind, with and without a path
  align         the whole dt_align call: cost, then both kinds with paths
  host          per pair, on --host-pairs pairs: the cost matrix from differences in float64 (torch.cdist without the Gram
                route, all of the job's CPU threads) and the same dynamic programme, vectorised over anti-diagonals in numpy,
                with the walk back; and that time scaled to the whole batch

Prints one JSON line per row; --out also appends them to a file.

  python tools/align_time.py [--reps 7] [--warmup 2] [--cases a,b] [--out profiles/align_time.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--cases", default="a,b")
ap.add_argument("--host-pairs", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

from distillation_trajectories_amd import _hip, engine   # noqa: E402
from distillation_trajectories_amd._hip import check, ptr, stream_ptr   # noqa: E402

CASES = {"a": dict(P=256, n=51, E=768), "b": dict(P=64, n=1001, E=3072)}
FP64_VECTOR_PEAK = 78.6e12          # MI355X datasheet, vector fp64
LINES = []


def emit(**row):
    line = json.dumps(row)
    print(line, flush=True)
    LINES.append(line)


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


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
    return stats(ms)


def host_dp(D, kind):
    """the recurrences of the header, one numpy step per anti-diagonal; returns (value, path length)"""
    n_a, n_b = D.shape
    C = np.full((n_a + 1, n_b + 1), np.inf)            # a border of +inf stands for the predecessors that do not exist
    pred = np.zeros((n_a, n_b), dtype=np.uint8)
    C[1, 1] = D[0, 0]
    for d in range(1, n_a + n_b - 1):
        i = np.arange(max(0, d - n_b + 1), min(n_a, d + 1))
        j = d - i
        diag, up, left = C[i, j], C[i, j + 1], C[i + 1, j]
        m, code = diag.copy(), np.zeros(len(i), dtype=np.uint8)
        pick = up < m
        m[pick], code[pick] = up[pick], 1
        pick = left < m
        m[pick], code[pick] = left[pick], 2
        C[i + 1, j + 1] = m + D[i, j] if kind == "dtw" else np.maximum(D[i, j], m)
        pred[i, j] = code
    i, j, length = n_a - 1, n_b - 1, 1
    while i or j:
        c = pred[i, j]
        i, j = (i - 1, j - 1) if c == 0 else (i - 1, j) if c == 1 else (i, j - 1)
        length += 1
    return float(C[n_a, n_b]), length


def host_case(name, X, Y, dev_out):
    """X, Y [n, P, E] on the host; the first --host-pairs pairs, checked against the device values"""
    pairs = min(args.host_pairs, X.shape[1])
    cost_s, dp_s = [], []
    for p in range(pairs):
        a, b = X[:, p].double(), Y[:, p].double()
        t0 = time.perf_counter()
        D = torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist").numpy()
        t1 = time.perf_counter()
        dtw, _ = host_dp(D, "dtw")
        fr, _ = host_dp(D, "frechet")
        t2 = time.perf_counter()
        cost_s.append(t1 - t0)
        dp_s.append(t2 - t1)
        for got, want in ((dtw, dev_out["dtw"][p].item()), (fr, dev_out["frechet"][p].item())):
            assert abs(got - want) <= 1e-9 * abs(want), (name, p, got, want)
    P = X.shape[1]
    per_pair = statistics.median(cost_s) + statistics.median(dp_s)
    emit(case=name, what="host", threads=torch.get_num_threads(), pairs_timed=pairs,
         cost_ms_per_pair=round(1e3 * statistics.median(cost_s), 2), dp_both_kinds_ms_per_pair=round(1e3 * statistics.median(dp_s), 2),
         batch_ms_scaled=round(1e3 * per_pair * P, 1))
    return 1e3 * per_pair * P


def run_case(name, P, n, E):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    Xh = torch.cumsum(torch.randn(n, P, E, generator=g) * 0.1, dim=0)
    Yh = torch.cumsum(torch.randn(n, P, E, generator=g) * 0.1, dim=0)
    Yh[0] = Xh[0]                                      # the shared start noise
    X, Y = Xh.to(dev), Yh.to(dev)
    lib = _hip.load()
    cells = n + n - 1
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    cost = torch.empty(P, n, n, **f64)
    status = torch.empty(P, **i32)
    val = {k: torch.empty(P, **f64) for k in ("dtw", "frechet")}
    path = {k: torch.empty(P, cells, 2, **i32) for k in ("dtw", "frechet")}
    plen = {k: torch.empty(P, **i32) for k in ("dtw", "frechet")}
    ws_dp = torch.empty(lib.dt_align_workspace_bytes(P, n, n, 1, 1), dtype=torch.uint8, device=dev)
    ws_all = torch.empty(lib.dt_align_workspace_bytes(P, n, n, 1, 0), dtype=torch.uint8, device=dev)
    rows = (ptr(X), n, X.stride(1), X.stride(0), ptr(Y), n, Y.stride(1), Y.stride(0), P, E)
    shape = dict(case=name, P=P, n_a=n, n_b=n, E=E, reps=args.reps, warmup=args.warmup)

    def cost_call():
        check(lib.dt_align_cost(*rows, ptr(cost), ptr(status), stream_ptr()), "dt_align_cost")

    t = timed(cost_call)
    flops = 3.0 * P * n * n * E
    rate = flops / (t["median_ms"] * 1e-3)
    emit(what="cost", **shape, **t, fp64_tflops=round(rate / 1e12, 2), share_of_vector_fp64_peak=round(rate / FP64_VECTOR_PEAK, 3),
         input_bytes=2 * P * n * E * 4, output_bytes=P * n * n * 8)
    for kind, code in (("dtw", engine.ALIGN_DTW), ("frechet", engine.ALIGN_FRECHET)):
        for with_path in (False, True):
            def dp_call():
                check(lib.dt_align_dp(ptr(cost), P, n, n, code, 0, ptr(val[kind]), ptr(path[kind]) if with_path else None,
                                      ptr(plen[kind]) if with_path else None, ptr(status), ptr(ws_dp), ws_dp.numel(),
                                      stream_ptr()), "dt_align_dp")
            emit(what="dp", kind=kind, path=with_path, **shape, **timed(dp_call), matrix_bytes=P * n * n * 8)

    def whole():
        check(lib.dt_align(*rows, 3, 0, None, ptr(val["dtw"]), ptr(val["frechet"]), ptr(path["dtw"]), ptr(plen["dtw"]),
                           ptr(path["frechet"]), ptr(plen["frechet"]), ptr(status), ptr(ws_all), ws_all.numel(),
                           stream_ptr()), "dt_align")

    t_all = timed(whole)
    emit(what="align", kinds="both", path=True, **shape, **t_all)
    assert status.sum().item() == 0
    host_ms = host_case(name, Xh, Yh, val)
    emit(case=name, what="host_over_device", ratio=round(host_ms / t_all["median_ms"], 1))


if not torch.cuda.is_available():
    sys.exit("align_time.py measures on the GPU; none is visible")
for c in args.cases.split(","):
    run_case(c, **CASES[c])
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
