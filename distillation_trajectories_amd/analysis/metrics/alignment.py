"""Which teacher step does a student step correspond to?  Dynamic time warping and the discrete Fréchet distance between a
teacher's and a student's trajectory (engine.device_align: csrc/dt_align.hip).

Every other trajectory metric pairs state i with state i, and for trajectories of different lengths the reference's
``interp1d`` branch (engine.device_resampled_distance) assumes that student time is a linear rescaling of teacher time.
The warping path measures that assumption instead: ``warp_deviation_*`` is how far the path strays from the straight line
in normalised time.  Beyond the reference, which has no alignment stage; no figures.
"""
import os

import numpy as np
import torch

from ... import engine
from .trajectory_metrics import _prepare, _stack_on_device


def path_summary(path, n_teacher, n_student):
    """Derived quantities of one warping path [L, 2] (cells (i, j), teacher step i with student step j):
    ``warp_deviation_mean`` / ``warp_deviation_max`` of |i / (nT - 1) - j / (nS - 1)| along it, and ``teacher_to_student``
    [nT], per teacher step the mean student step it is aligned with (NaN for a step the path does not visit, that is for
    an empty path)."""
    path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    t2s = np.full(n_teacher, np.nan)
    if len(path) == 0:
        return {"warp_deviation_mean": float("nan"), "warp_deviation_max": float("nan"), "teacher_to_student": t2s}
    dev = np.abs(path[:, 0] / (n_teacher - 1) - path[:, 1] / (n_student - 1))
    hits = np.bincount(path[:, 0], minlength=n_teacher)
    sums = np.bincount(path[:, 0], weights=path[:, 1], minlength=n_teacher)
    t2s[hits > 0] = sums[hits > 0] / hits[hits > 0]
    return {"warp_deviation_mean": float(dev.mean()), "warp_deviation_max": float(dev.max()), "teacher_to_student": t2s}


def _host(out):
    """one device-to-host copy per output tensor"""
    return {k: v.cpu().numpy() for k, v in out.items()}


def _pair_result(host, s, n_teacher, n_student, with_cost):
    dtw_len, fr_len = int(host["dtw_path_len"][s]), int(host["frechet_path_len"][s])
    dtw_path = host["dtw_path"][s, :dtw_len].copy()
    dtw = float(host["dtw"][s])
    res = {"dtw_distance": dtw, "dtw_normalized": dtw / dtw_len if dtw_len else float("nan"),
           "frechet_distance": float(host["frechet"][s]), "dtw_path": dtw_path,
           "frechet_path": host["frechet_path"][s, :fr_len].copy(), "status": int(host["status"][s])}
    res.update(path_summary(dtw_path, n_teacher, n_student))
    if with_cost:
        res["cost_matrix"] = host["cost"][s].copy()
    return res


def align_trajectories(teacher_trajectory, student_trajectory, band=0, cost_matrix=False):
    """Alignment of one (teacher, student) pair in the reference's trajectory forms (lists of tensors or of (tensor, t)
    tuples, as ``compute_trajectory_metrics`` takes them; a student of another resolution is resized to the teacher's).
    Every list entry is one state.  Returns Python / numpy values: ``dtw_distance``, ``dtw_normalized`` (distance / path
    length), ``frechet_distance``, ``dtw_path`` and ``frechet_path`` [L, 2], ``warp_deviation_mean``,
    ``warp_deviation_max``, ``teacher_to_student`` [nT] (``path_summary`` of the DTW path), ``status`` (0 ok, 1 non-finite
    states: NaN distances and empty paths) and, with ``cost_matrix``, the [nT, nS] matrix of distances.  ``band``: 0, or a
    Sakoe-Chiba band in steps of the longer trajectory."""
    X, Y, device = _prepare(teacher_trajectory, student_trajectory)
    Xd, Yd = _stack_on_device(X, device), _stack_on_device(Y, device)
    if Xd.shape[2] != Yd.shape[2]:
        raise ValueError(f"teacher states have {Xd.shape[2]} elements, student states {Yd.shape[2]}")
    out = engine.device_align(Xd, Yd, kind="both", band=band, path=True, cost=cost_matrix)
    return _pair_result(_host(out), 0, len(X), len(Y), cost_matrix)


def alignment_pairs(X, Y, band=0, cost_matrix=False, layout="step"):
    """The same for device trajectories X [nT, S, ...] and Y [nS, S, ...] (or [S, n, ...] with ``layout="problem"``), one
    pair per sample s: ONE ``engine.device_align`` call, then only values, paths and statuses leave the device.  Returns
    numpy arrays: ``dtw_distance``, ``dtw_normalized``, ``frechet_distance``, ``warp_deviation_mean``,
    ``warp_deviation_max`` [S], ``teacher_to_student`` [S, nT], ``dtw_path`` / ``frechet_path`` [S, nT+nS-1, 2] (-1 past
    ``dtw_path_len`` / ``frechet_path_len`` [S]), ``status`` [S] and, with ``cost_matrix``, ``cost_matrix`` [S, nT, nS]."""
    out = engine.device_align(X, Y, kind="both", band=band, path=True, cost=cost_matrix, layout=layout)
    host = _host(out)
    S = host["status"].shape[0]
    n_t, n_s = (t.shape[1] if layout == "problem" and t.dim() > 2 else t.shape[0] for t in (X, Y))
    rows = [_pair_result(host, s, n_t, n_s, False) for s in range(S)]
    res = {k: np.array([r[k] for r in rows]) for k in ("dtw_distance", "dtw_normalized", "frechet_distance",
                                                       "warp_deviation_mean", "warp_deviation_max", "teacher_to_student")}
    for k in ("dtw_path", "frechet_path", "dtw_path_len", "frechet_path_len", "status"):
        res[k] = host[k]
    if cost_matrix:
        res["cost_matrix"] = host["cost"]
    return res


def alignment_sweep(teacher_model, student_models, config, seeds, student_steps, band=0, output_dir=None):
    """Alignment of every student with one teacher, for every step count of ``student_steps``.  Trajectories come from
    ``TrajectoryManager``'s batched device loop: per seed the CPU generator is seeded, the start noise drawn and then one
    draw per update, shared by the teacher and every student (``generate_trajectories_batched``); the teacher runs once
    with ``config.teacher_steps``.  One ``engine.device_align`` call per (student, step count); the states stay on the
    device.  Returns {(student index, steps): ``alignment_pairs`` result} and writes each as
    ``alignment_student_{k}_steps_{n}.npz`` under ``output_dir`` (default ``config.analysis_dir``/alignment)."""
    from ...utils.trajectory_manager import TrajectoryManager, timestep_list
    students, seeds, step_counts = list(student_models), list(seeds), list(student_steps)
    if not students or not seeds or not step_counts:
        raise ValueError("alignment_sweep needs at least one student model, one seed and one step count")
    for n in step_counts:
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= config.sample_steps:
            raise ValueError(f"student_steps entry {n!r} must be an int in [1, sample_steps = {config.sample_steps}]")
    shape = (config.channels, config.image_size, config.image_size)
    for m in students:
        if getattr(m, "image_size", config.image_size) != config.image_size:
            raise ValueError("alignment_sweep shares the start noise: every student needs the teacher's resolution")
    t_idx = timestep_list(config.sample_steps, config.teacher_steps)
    s_idx = {n: timestep_list(config.sample_steps, int(n)) for n in step_counts}
    updates = lambda idx: sum(1 for t in idx if t > 0)
    n_z = max([updates(t_idx)] + [updates(i) for i in s_idx.values()])
    if min([updates(t_idx)] + [updates(i) for i in s_idx.values()]) < 1:
        raise ValueError("an alignment needs at least two states on both sides")
    x0, z = [], []
    for seed in seeds:
        torch.manual_seed(seed)
        np.random.seed(seed)
        x0.append(torch.randn(1, *shape))
        z.append(torch.stack([torch.randn(1, *shape) for _ in range(n_z)]))
    x0 = torch.cat(x0)
    zz = torch.stack(z, dim=1).reshape(n_z, len(seeds), -1)
    if output_dir is None:
        output_dir = os.path.join(config.analysis_dir, "alignment")
    os.makedirs(output_dir, exist_ok=True)
    teacher_model.eval()
    t_states, _ = TrajectoryManager(teacher_model, teacher_model, config)._run_states(teacher_model, x0, t_idx,
                                                                                      zz[:updates(t_idx)])
    results = {}
    for k, student in enumerate(students):
        student.eval()
        manager = TrajectoryManager(teacher_model, student, config)
        for n in step_counts:
            s_states, _ = manager._run_states(student, x0, s_idx[n], zz[:updates(s_idx[n])])
            res = alignment_pairs(t_states, s_states, band=band)
            res["seeds"] = np.array(seeds)
            res["teacher_timesteps"] = np.array(t_idx[:t_states.shape[0]])
            res["student_timesteps"] = np.array(s_idx[n][:s_states.shape[0]])
            np.savez(os.path.join(output_dir, f"alignment_student_{k}_steps_{int(n)}.npz"), **res)
            results[(k, int(n))] = res
    return results
