#!/usr/bin/env python3
"""Times of the editing stage on one MI355X.

  loops : the masked sampler loop (dt_sample_trajectory_masked, a rectangular mask, known rows through a row table) against
          the unmasked loop (dt_sample_trajectory) of the same shape -- ENGINE rule, T = 50 steps, batch 64 at 16 x 16 x 3 --
          on the fused path (sf 0.1, sf 0.2) and on the layered path (the same models with the fused kernel off, and sf 0.5).
          The two are alternated --reps times after one warm-up call each; every call is bracketed by device events on the
          stream and ends in a synchronise.  Printed: median, min and max of each, so the run-to-run spread stands beside the
          difference.  ``--root DIR`` imports the package from another checkout (one that has no masked loop prints the
          unmasked times only): the unmasked loop of the parent commit is the yardstick for "the blend is free".
  sweep : ``inpainting_sweep`` (teacher sf 0.5, students sf 0.1 and sf 0.2, T = 20, 2 images x 2 masks x 4 samples) against
          the same 16 cells as B = 1 ``inpaint_with_trajectory`` calls per model; host clock around work that ends in a
          synchronise, median / min / max of --reps calls after one warm-up call.

Prints one JSON line per case; --out also writes them to a file.

  python tools/edit_time.py [--reps 7] [--root DIR] [--out profiles/edit_time.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("--label", default="this")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch   # noqa: E402

from distillation_trajectories_amd import engine                      # noqa: E402
from distillation_trajectories_amd._hip import COND_NONE, RULE_ENGINE   # noqa: E402
from distillation_trajectories_amd.analysis.trajectory_engine import engine_coefficients   # noqa: E402
from distillation_trajectories_amd.config import Config               # noqa: E402
from distillation_trajectories_amd.models import DiffusionUNet        # noqa: E402
from distillation_trajectories_amd.synthetic import make_model        # noqa: E402

DEV = torch.device("cuda:0")
T, B, E = 50, 64, 768
LINES = []


def emit(**row):
    line = json.dumps(dict(label=args.label, **row))
    print(line, flush=True)
    LINES.append(line)


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def config(T_):
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, T_
    return cfg


def loop_case(sf, fused):
    m = make_model(DiffusionUNet, config(T), sf).to(DEV)
    h = engine.UNetHandle.for_module(m)
    h.set_fused(fused)
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(B, E, generator=g).to(DEV)
    z = torch.randn(T + B, E, generator=g).to(DEV)
    known = (torch.rand(4, E, generator=g) * 2 - 1).to(DEV)
    mask = torch.zeros(1, 3, 16, 16)
    mask[:, :, 4:12, 3:13] = 1
    mask = mask.reshape(1, E).to(DEV)
    mrow = torch.zeros(B, dtype=torch.int32, device=DEV)
    krow = (torch.arange(B) % 4).to(torch.int32).to(DEV)
    order = list(range(T - 1, -1, -1))
    coefs = engine_coefficients(T)
    cs, noise = [coefs[t] for t in order], [t > 0 for t in order]
    tb = h.time_bias(order, [COND_NONE] * T)
    traj = torch.empty(T + 1, B, E, device=DEV)
    traj[0] = x0
    masked = hasattr(h, "sample_masked")

    def run(which):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if which:
            h.sample_masked(RULE_ENGINE, traj, 16, 16, tb, 1, cs, noise, mask, known, mrow, krow, z=z, z_shift=order)
        else:
            h.sample(RULE_ENGINE, traj, 16, 16, tb, 1, cs, noise, z=z, z_shift=order)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    kinds = (0, 1) if masked else (0,)
    for k in kinds:
        run(k)
    ms = {k: [] for k in kinds}
    for _ in range(args.reps):
        for k in kinds:
            ms[k].append(run(k))
    row = dict(case="loop", sf=sf, path="fused" if h.fused_active(16, 16) else "layered", T=T, batch=B, reps=args.reps,
               unmasked=stats(ms[0]))
    if masked:
        row["masked"] = stats(ms[1])
        row["masked_over_unmasked"] = round(row["masked"]["median_ms"] / row["unmasked"]["median_ms"], 4)
    emit(**row)


def sweep_case():
    from distillation_trajectories_amd.editing import inpainting_sweep, masked_inpainting
    from distillation_trajectories_amd.utils.diffusion import get_diffusion_params
    Ts, S = 20, 4
    cfg = config(Ts)
    teacher = make_model(DiffusionUNet, cfg, 0.5).to(DEV)
    students = [make_model(DiffusionUNet, cfg, sf).to(DEV) for sf in (0.1, 0.2)]
    g = torch.Generator().manual_seed(2)
    images = torch.rand(2, 3, 16, 16, generator=g)
    masks = [torch.zeros(16, 16), torch.zeros(16, 16)]
    masks[0][4:11, 3:12] = 1
    masks[1][2:14, 6:10] = 1
    dp = get_diffusion_params(Ts, cfg)

    def batched():
        inpainting_sweep(teacher, students, cfg, images, masks, S)

    def singles():
        for m in [teacher] + students:
            for i in range(2):
                for j in range(2):
                    for s in range(S):
                        torch.manual_seed(42 + s)
                        mask = masked_inpainting.normalize_mask(masks[j], 3, DEV)
                        masked_inpainting.inpaint_with_trajectory(m, dp, images[i:i + 1].to(DEV), mask, cfg, DEV)

    out = {}
    for name, fn in (("sweep", batched), ("single_calls", singles)):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = stats(ms)
    emit(case="inpainting_sweep", T=Ts, cells=16, models=3, reps=args.reps,
         single_over_sweep=round(out["single_calls"]["median_ms"] / out["sweep"]["median_ms"], 2), **out)


if not torch.cuda.is_available():
    sys.exit("edit_time.py measures on the GPU; none is visible")
for sf, fused in ((0.1, True), (0.2, True), (0.1, False), (0.2, False), (0.5, False)):
    loop_case(sf, fused)
try:
    import distillation_trajectories_amd.editing   # noqa: F401
    have_editing = True
except ImportError:
    have_editing = False
if have_editing:
    sweep_case()
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
