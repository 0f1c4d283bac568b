#!/usr/bin/env python3
"""Times of the spatial-frequency spectra (include/dt_hip_spectral.h) on one MI355X.

Three picture sizes, 16 x 16, 32 x 32 and 64 x 64, each with C = 3 and 51 x 256 rows (a 50-step trajectory of 256 samples)
of a teacher and a student set.  For each, after --warmup calls, --reps calls bracketed by device events on the stream and
ended by a synchronise (the events' own clock; the board's clocks are neither set nor read: they are what the machine runs at
under this load); median, min and max are printed:

  pair          engine.device_spectral_pair with the sample sums: the table sort, one workgroup per row, the sums; with it
                the fp64 rate of the direct DFT as the kernel does it (three transforms of the columns v <= W/2 per channel:
                2 W fused multiply-adds per cell along x, 4 H along y; a fused multiply-add counted as 2 FLOP) and its
                share of the datasheet's vector fp64 peak (78.6 TFLOP/s)
  power         engine.device_spectrum of the teacher set alone
  torch_fft     what a user would otherwise write: torch.fft.fft2 of the float64 copies of both sets and of their
                difference on the device, the five per-cell products, and the same binning by index_add_.  The time
                yardstick; its values are also compared with the stage's (largest relative difference per output)
  numpy_16      the same with numpy.fft.fft2 and bincount on --host-rows rows, on 16 host threads, scaled to all rows

Prints one JSON line per row; --out also appends them to a file.

  python tools/spectral_time.py [--reps 10] [--warmup 2] [--sizes 16,32,64] [--out profiles/spectral_time.txt]
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
ap.add_argument("--sizes", default="16,32,64")
ap.add_argument("--states", type=int, default=51)
ap.add_argument("--samples", type=int, default=256)
ap.add_argument("--host-rows", type=int, default=512)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

from distillation_trajectories_amd import engine   # noqa: E402

C = 3
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


def torch_pair(X, Y, H, table, n_bins):
    """[n, C, n_bins, 5] float64: the stage's sample sums by torch.fft in float64"""
    n, S = X.shape[:2]
    x, y = X.view(n, S, C, H, H).double(), Y.view(n, S, C, H, H).double()
    A, B, D = torch.fft.fft2(x), torch.fft.fft2(y), torch.fft.fft2(x - y)
    cross = A * B.conj()
    cells = torch.stack([A.real ** 2 + A.imag ** 2, B.real ** 2 + B.imag ** 2, cross.real, cross.imag,
                         D.real ** 2 + D.imag ** 2], dim=-1).sum(dim=1)                           # [n, C, H, H, 5]
    out = torch.zeros(n, C, n_bins, 5, dtype=torch.float64, device=X.device)
    return out.index_add_(2, table.view(-1).long(), cells.view(n, C, H * H, 5))


def numpy_pair(x, y, table, n_bins):
    """the same for host arrays [rows, C, H, H] float32, one worker's share: [C, n_bins, 5]"""
    x, y = x.astype(np.float64), y.astype(np.float64)
    A, B, D = np.fft.fft2(x), np.fft.fft2(y), np.fft.fft2(x - y)
    cross = A * B.conj()
    cells = np.stack([np.abs(A) ** 2, np.abs(B) ** 2, cross.real, cross.imag, np.abs(D) ** 2], axis=-1).sum(axis=0)
    out = np.zeros((C, n_bins, 5))
    for c in range(C):
        for q in range(5):
            out[c, :, q] = np.bincount(table.ravel(), weights=cells[c, :, :, q].ravel(), minlength=n_bins)
    return out


def run_size(H):
    from concurrent.futures import ThreadPoolExecutor
    dev = torch.device("cuda:0")
    n, S, E = args.states, args.samples, C * H * H
    g = torch.Generator(device="cpu").manual_seed(H)
    X = torch.randn(n, S, E, generator=g).to(dev)
    Y = (X + 0.1 * torch.randn(n, S, E, generator=g).to(dev)).contiguous()
    table_host, cells = engine.radial_bins(H, H)
    table, n_bins = torch.from_numpy(table_host).to(dev), len(cells)
    shape = dict(H=H, W=H, C=C, states=n, samples=S, n_bins=n_bins, reps=args.reps, warmup=args.warmup)

    t = timed(lambda: engine.device_spectral_pair(X, Y, C, H, H, sum_samples=True))
    flops = 2.0 * n * S * C * 3 * (H * (H // 2 + 1)) * (2 * H + 4 * H)
    rate = flops / (t["median_ms"] * 1e-3)
    emit(what="pair", **shape, **t, input_bytes=8 * n * S * E, dft_fp64_tflops=round(rate / 1e12, 2),
         share_of_vector_fp64_peak=round(rate / FP64_VECTOR_PEAK, 3))
    emit(what="power", **shape, **timed(lambda: engine.device_spectrum(X, C, H, H, sum_samples=True)))
    tt = timed(lambda: torch_pair(X, Y, H, table, n_bins))
    emit(what="torch_fft", **shape, **tt, hand_written_over_torch=round(t["median_ms"] / tt["median_ms"], 3),
         torch_peak_bytes=torch.cuda.max_memory_allocated())

    got = engine.device_spectral_pair(X, Y, C, H, H, sum_samples=True)
    assert not got["status"].any().item() and (got["count"] == S).all().item()
    mine = torch.cat([got["power_a"].unsqueeze(-1), got["power_b"].unsqueeze(-1), got["cross"], got["error"].unsqueeze(-1)], dim=-1)
    theirs = torch_pair(X, Y, H, table, n_bins)
    scale = theirs.abs().amax(dim=(0, 1, 2)).clamp_min(1e-300)
    scale[3] = scale[2]                                     # the imaginary cross term cancels in a radial bin: against C_re
    emit(what="values", H=H, largest_difference_over_largest_value=[float(f"{v:.3g}") for v in
                                                                   ((mine - theirs).abs().amax(dim=(0, 1, 2)) / scale).tolist()])

    rows = min(args.host_rows, n * S)
    xh, yh = (t_.view(n * S, C, H, H)[:rows].cpu().numpy() for t_ in (X, Y))
    parts = np.array_split(np.arange(rows), 16)
    with ThreadPoolExecutor(max_workers=16) as pool:
        def once():
            t0 = time.perf_counter()
            sum(pool.map(lambda idx: numpy_pair(xh[idx], yh[idx], table_host, n_bins), parts))
            return (time.perf_counter() - t0) * 1e3
        once()
        ms = [once() for _ in range(3)]
    scaled = statistics.median(ms) * n * S / rows
    emit(what="numpy_16", H=H, host_rows=rows, threads=16, median_ms_for_host_rows=round(statistics.median(ms), 3),
         scaled_to_all_rows_ms=round(scaled, 1), hand_written_over_numpy=round(t["median_ms"] / scaled, 5))


if not torch.cuda.is_available():
    sys.exit("spectral_time.py measures on the GPU; none is visible")
for size in args.sizes.split(","):
    run_size(int(size))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
