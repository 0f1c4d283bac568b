#!/usr/bin/env python3
"""Times of sampler noise on one MI355X: the torch CPU generator plus upload against the same numbers made on the device.

  stage   : the noise stage of ``fid_score.generate_samples`` in both modes, for n samples of T steps at C x H x H -- "host":
            the reference's draw order on the CPU generator (start of sample i, then its T - 1 steps), the stack into the
            step-major [T - 1][n][E] table and its upload, as the function does it; "device": ``engine.HostGenerator()`` +
            ``engine.device_randn`` into the [T][n][E] buffer, the end state read back into the CPU generator.  Host clock
            around work that ends in a device synchronise; the two are alternated --reps times after one warm-up call each,
            both from the same generator state.  Printed: median, min and max of each, their ratio, and whether the two
            tables are equal bit for bit at the timed size.
  kernels : the two kernels alone: dt_rng_mt19937_words for one stream and for 256 streams (words per second),
            dt_rng_normal_from_words over a word buffer (normals per second, and the bytes per second of the words it reads
            plus the normals it writes).  One timed window is device events around ``launches`` back-to-back launches (chosen
            so that a window is of the order of 0.1 s), --reps windows after a warm-up window; the time printed is per launch.
            The launches of a window rotate through four input / output buffer sets, 1.6 GB in all for the transform, so that
            no launch finds its words in the 256 MB last-level cache from the launch before.

Prints one JSON line per case; --out also writes them to a file (replacing it).

  python tools/rng_time.py [--reps 5] [--out profiles/rng_time.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("--label", default="this")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch   # noqa: E402

from distillation_trajectories_amd import _hip, engine   # noqa: E402

DEV = torch.device("cuda:0")
LINES = []


def emit(**row):
    line = json.dumps(dict(label=args.label, **row))
    print(line, flush=True)
    LINES.append(line)


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def host_stage(n, T, C, H):
    """generate_samples' host noise: draws in the reference's order, the step-major table, the upload"""
    starts, zs = [], []
    for _ in range(n):
        x = torch.randn(1, C, H, H)
        starts.append(x)
        zs.append(torch.stack([torch.randn(x.shape) for _ in range(T - 1)]))
    x0 = torch.cat(starts)
    z = torch.stack(zs, dim=1).reshape(T - 1, n, -1)
    return x0.reshape(n, -1).to(DEV), z.reshape(-1, z.shape[-1]).to(DEV)


def device_stage(n, T, C, H):
    E = C * H * H
    buf = torch.empty(T, n, E, dtype=torch.float32, device=DEV)
    engine.device_randn(state=engine.HostGenerator(), draws=(n, T), E=E, out=buf, strides=(0, E, n * E), device=DEV)
    return buf[0], buf[1:].reshape(-1, E)


def stage_case(n, T, C, H):
    torch.manual_seed(1234)
    start = torch.get_rng_state()
    runs = {"host": host_stage, "device": device_stage}
    ms, last, end_state = {k: [] for k in runs}, {}, {}
    for rep in range(args.reps + 1):          # rep 0 warms both up
        for name, fn in runs.items():
            torch.set_rng_state(start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(n, T, C, H)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                ms[name].append(dt)
            last[name], end_state[name] = out, torch.get_rng_state()
    equal = all(torch.equal(a, b) for a, b in zip(last["host"], last["device"])) and \
        torch.equal(end_state["host"], end_state["device"])
    normals = n * T * C * H * H
    row = dict(case="noise_stage", n=n, T=T, shape=[C, H, H], normals=normals, reps=args.reps,
               cpu_capability=torch.backends.cpu.get_cpu_capability(), torch_threads=torch.get_num_threads(),
               host=stats(ms["host"]), device=stats(ms["device"]), equal_bits_and_state=bool(equal))
    row["host_over_device"] = round(row["host"]["median_ms"] / row["device"]["median_ms"], 2)
    row["host_normals_per_s"] = round(normals / row["host"]["median_ms"] * 1e3)
    row["device_normals_per_s"] = round(normals / row["device"]["median_ms"] * 1e3)
    emit(**row)


SETS = 4      # buffer sets a window rotates through


def timed(fn, launches):
    """per-launch milliseconds of --reps windows of ``launches`` calls fn(i), after one warm-up window"""
    ms = []
    for rep in range(args.reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(launches):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(a.elapsed_time(b) / launches)
    return ms


def words_case(streams, n, launches):
    outs = [torch.empty(streams, n, dtype=torch.int32, device=DEV) for _ in range(SETS)]
    lib = _hip.load()
    seeds = torch.arange(streams, dtype=torch.int64, device=DEV)

    def run(i):
        _hip.check(lib.dt_rng_mt19937_words(_hip.ptr(seeds), None, None, streams, 0, n, _hip.ptr(outs[i % SETS]), n, None, None,
                                            _hip.stream_ptr()), "dt_rng_mt19937_words")
    ms = timed(run, launches)
    row = dict(case="mt19937_words", streams=streams, words_per_stream=n, launches_per_window=launches, reps=args.reps,
               **stats(ms))
    row["words_per_s"] = round(streams * n / row["median_ms"] * 1e3)
    emit(**row)


def transform_case(E, draws, launches):
    lib = _hip.load()
    W = E if E % 16 == 0 else E + 16
    words = [engine.device_mt19937_words(seeds=range(64 * k, 64 * k + 64), n=draws * W // 64, device=DEV).reshape(1, -1)
             for k in range(SETS)]
    outs = [torch.empty(draws, E, dtype=torch.float32, device=DEV) for _ in range(SETS)]

    def run(i):
        w, o = words[i % SETS], outs[i % SETS]
        _hip.check(lib.dt_rng_normal_from_words(_hip.ptr(w), w.shape[1], 1, draws, 1, E, _hip.ptr(o), 0, E, E,
                                                _hip.stream_ptr()), "dt_rng_normal_from_words")
    ms = timed(run, launches)
    row = dict(case="normal_from_words", E=E, draws=draws, normals=draws * E, launches_per_window=launches,
               buffer_sets=SETS, reps=args.reps, **stats(ms))
    row["normals_per_s"] = round(draws * E / row["median_ms"] * 1e3)
    row["bytes_per_s"] = round(4 * (draws * W + draws * E) / row["median_ms"] * 1e3)
    emit(**row)


if not torch.cuda.is_available():
    sys.exit("rng_time.py measures on the GPU; none is visible")
with torch.cuda.device(DEV):
    words_case(1, 1 << 24, 8)
    words_case(256, 1 << 18, 200)
    transform_case(768, 64 * 1024, 400)
    transform_case(105, 512 * 1024, 400)
    stage_case(2048, 50, 3, 16)
    stage_case(512, 50, 3, 32)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
