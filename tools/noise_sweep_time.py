#!/usr/bin/env python3
"""Wall time of the noise-prediction analysis on the device against the per-timestep loop a reference caller runs today.

  driver : analyze_noise_prediction (10 t x 10 images, teacher sf 1.0 vs student sf 0.5) at 16 x 16 and 32 x 32
  sweep  : noise_prediction_sweep over every t of configs[2] (T = 50, 16 x 16) x 10 images x its 11 students

The baseline of both is the same work done per timestep with the existing pieces, as the reference's driver does it
(analysis/noise_prediction/noise_analysis.py:238-286): randn_like, the torch noising expression, predict_noise for the
teacher and for the student, calculate_noise_metrics -- for every student, the teacher recomputed each time.  Times are
medians of --reps runs after one warm-up run (launch plans settled, workspaces allocated); the GPU is synchronised around
each run.  Prints one JSON line per case.

  python tools/noise_sweep_time.py [--reps 5]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

from distillation_trajectories_amd.analysis.noise_prediction import noise_analysis as na   # noqa: E402
from distillation_trajectories_amd.config import Config   # noqa: E402
from distillation_trajectories_amd.models import DiffusionUNet   # noqa: E402
from distillation_trajectories_amd.synthetic import make_model   # noqa: E402

DEV = torch.device("cuda:0")
SIZES = [0.01, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def loop_pieces(teacher, students, images, t_list, cfg):
    """The per-timestep loop of the reference driver on the existing pieces: {sf: {t: metrics}}."""
    out = {}
    coef = na.noise_coefficients(cfg, t_list).to(DEV)
    B = images.shape[0]
    for sf, student in students.items():
        out[sf] = {}
        for i, t in enumerate(t_list):
            tt = torch.full((B,), t, device=DEV, dtype=torch.long)
            noise = torch.randn_like(images)
            noisy = coef[i, 0] * images + coef[i, 1] * noise
            te = na.predict_noise(teacher, noisy, tt, DEV)
            se = na.predict_noise(student, noisy, tt, DEV)
            out[sf][t] = na.calculate_noise_metrics(te, se)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    cfg = Config()
    models = {sf: make_model(DiffusionUNet, cfg, sf).to(DEV) for sf in SIZES}
    teacher = models[1.0]
    g = torch.Generator().manual_seed(0)
    tmp = tempfile.mkdtemp(prefix="noise_sweep_time_")

    for H in (16, 32):
        c = Config()
        c.image_size, c.timesteps = H, 50
        images = (torch.rand(10, 3, H, H, generator=g) * 2 - 1).to(DEV)
        t_list = torch.linspace(0, c.timesteps - 1, 10, dtype=torch.long).tolist()

        def driver():
            with contextlib.redirect_stdout(io.StringIO()):
                return na.analyze_noise_prediction(teacher, models[0.5], c, output_dir=tmp, size_factor=0.5, fixed_samples=images)
        torch.manual_seed(1)
        t_drv, res = timed(driver, args.reps)
        torch.manual_seed(1)
        t_loop, ref = timed(lambda: loop_pieces(teacher, {0.5: models[0.5]}, images, t_list, c), args.reps)
        # same seed, same draw order: the two agree up to the forwards' batch-shape rounding
        worst = max(abs(res["metrics_by_timestep"][t][k] - ref[0.5][t][k]) / max(abs(ref[0.5][t][k]), 1e-12)
                    for t in t_list for k in ("mse", "mae", "cosine_similarity"))
        print(json.dumps(dict(case="driver", H=H, timesteps=10, images=10, teacher_sf=1.0, student_sf=0.5,
                              device_ms=round(1e3 * t_drv, 3), loop_ms=round(1e3 * t_loop, 3),
                              speedup=round(t_loop / t_drv, 2), max_rel_diff=worst)), flush=True)

    c = Config()
    c.image_size, c.timesteps = 16, 50
    images = (torch.rand(10, 3, 16, 16, generator=g) * 2 - 1).to(DEV)
    students = {sf: models[sf] for sf in SIZES}
    t_list = list(range(c.timesteps))
    torch.manual_seed(2)
    t_sw, sw = timed(lambda: na.noise_prediction_sweep(teacher, students, images, config=c, true_noise_metrics=False), args.reps)
    torch.manual_seed(2)
    t_swt, _ = timed(lambda: na.noise_prediction_sweep(teacher, students, images, config=c), args.reps)
    torch.manual_seed(2)
    t_loop, ref = timed(lambda: loop_pieces(teacher, students, images, t_list, c), args.reps)
    print(json.dumps(dict(case="dense_sweep", H=16, timesteps=c.timesteps, images=10, students=len(students), teacher_sf=1.0,
                          rows_per_chunk=na.SWEEP_CHUNK_ROWS, device_ms=round(1e3 * t_sw, 3),
                          device_ms_with_true_noise=round(1e3 * t_swt, 3), loop_ms=round(1e3 * t_loop, 3),
                          speedup=round(t_loop / t_sw, 2))), flush=True)


if __name__ == "__main__":
    main()
