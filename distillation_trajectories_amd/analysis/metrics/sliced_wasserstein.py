"""At which reverse step does the student's DISTRIBUTION of states leave the teacher's, and by how much more than two
independent draws from the teacher differ?  The sliced Wasserstein distance between the set of the teacher's states and the
set of the student's states at a step (engine.device_swd: csrc/dt_swd.hip): both sets are projected onto L random unit
directions, and the exact 1-D Wasserstein distance W_p between the projections is averaged over the directions
(``swd`` = (mean_l W_p^p)^(1/p)) or maximised (``max_swd``, with the direction that separates the sets most).

It needs no network and no weights, works at every step and resolution, and is a metric between distributions; the other
set-level stages (FID, KID, precision / recall) mean something for finished pictures only, and ``dt_traj_wasserstein`` is a
marginal over the coordinates of ONE pair of states.  Beyond the reference, which has no such stage; no figures."""
import os

import numpy as np
import torch

from ... import engine
from .spectral import _state_view
from .trajectory_metrics import _prepare


def derived_distances(mean_w, max_w, p):
    """(swd, max_swd) = (mean_w ** (1/p), max_w ** (1/p)) in float64 (NaN stays NaN)."""
    mean_w, max_w = np.asarray(mean_w, dtype=np.float64), np.asarray(max_w, dtype=np.float64)
    if p == 1:
        return mean_w.copy(), max_w.copy()
    if p == 2:
        return np.sqrt(mean_w), np.sqrt(max_w)
    raise ValueError(f"p={p!r} must be 1 or 2")


def _distances(X, Y, directions, n_directions, p, seed):
    out = engine.device_swd(X, Y, directions=directions, n_directions=n_directions, p=p, seed=seed)
    swd, max_swd = derived_distances(out["mean_w"].cpu().numpy(), out["max_w"].cpu().numpy(), p)
    return {"swd": swd, "max_swd": max_swd, "argmax": out["argmax"].cpu().numpy(), "status": out["status"].cpu().numpy()}


def sliced_wasserstein_pairs(X, Y, directions=None, n_directions=512, p=2, seed=0):
    """Sliced Wasserstein distance between the sets of X (teacher) and of Y (student), state by state: device tensors
    [n, S, E] float32 (state i holds a set of S rows; views are read in place; the set sizes of X and Y may differ; [S, E]
    is one state), or the ``engine.SwdSorted`` of a set whose sorted projections are already made.  ONE
    ``engine.device_swd`` call, then the p-th root in numpy float64.  Returns ``swd`` [n] = (mean over the directions of
    W_p^p)^(1/p), ``max_swd`` [n] = the largest W_p over the directions, ``argmax`` [n] (that direction's index, -1 for a
    flagged state), ``status`` [n] (1: a NaN or Inf in the state or the directions, its distances are NaN) and
    ``directions`` [L, E] float32 (``engine.swd_directions(E, n_directions, seed)`` unless given)."""
    res = _distances(X, Y, directions, n_directions, p, seed)
    if directions is None:
        made = [s.directions for s in (X, Y) if isinstance(s, engine.SwdSorted)]
        width = (X if isinstance(X, torch.Tensor) else Y).shape[-1] if not made else None
        directions = made[0] if made else engine.swd_directions(width, n_directions, seed)
    res["directions"] = directions.detach().cpu().numpy()
    return res


def sliced_wasserstein_trajectories(teacher_trajectory, student_trajectory, directions=None, n_directions=512, p=2, seed=0):
    """The same for one (teacher, student) pair in the reference's trajectory forms (lists of tensors [B, C, H, W] or of
    (tensor, t) tuples, as ``align_trajectories`` takes them; a student of another resolution is resized to the
    teacher's).  State i of the teacher meets state i of the student: the lengths must be equal.  The B pictures of an
    entry are its set; the student's B may differ from the teacher's."""
    if len(teacher_trajectory) != len(student_trajectory):
        raise ValueError(f"the teacher has {len(teacher_trajectory)} states, the student {len(student_trajectory)}: "
                         "the distance pairs them one to one")
    X, Y, device = _prepare(teacher_trajectory, student_trajectory)
    for images in (X, Y):
        if images[0].dim() != 4 or any(x.shape != images[0].shape for x in images):
            raise ValueError("every state of a trajectory must be a tensor [B, C, H, W] of one shape")
    if X[0].shape[1:] != Y[0].shape[1:]:
        raise ValueError(f"teacher states are {tuple(X[0].shape[1:])}, student states {tuple(Y[0].shape[1:])}")
    stack = lambda images: torch.stack([im.detach().reshape(im.shape[0], -1) for im in images]).to(device=device, dtype=torch.float32)
    return sliced_wasserstein_pairs(stack(X), stack(Y), directions, n_directions, p, seed)


def sliced_wasserstein_sweep(teacher_model, student_models, config, guidance_scales, num_samples, every=1, n_directions=512, p=2,
                             output_dir=None):
    """Sliced Wasserstein distances of every student against one teacher, for every guidance scale and state.  The
    trajectories come from ``sample_grid`` exactly as ``spectral_sweep`` runs it (``noise_table(42, ...)``, sample s from
    seed 42 + s); the teacher is sampled once for all scales, every ``every``-th state plus the last is taken
    (``perceptual.state_indices``), and the teacher's sorted projections are made once per scale and shared by all
    students.  Three quantities per (student, scale, state), which answer different questions:

    ``swd``        all of the teacher's samples against all of the student's.  Sample s of both starts from the same seed, so
                   this is a PAIRED comparison: it is exactly 0 for a student that reproduces the teacher, and it does not
                   contain the sampling noise of two independent draws.
    ``swd_split``  the teacher's even-numbered samples against the student's odd-numbered ones: disjoint seeds, two
                   independent draws.  This is the number to hold against ``floor``.
    ``floor``      the teacher's even-numbered samples against the teacher's own odd-numbered ones: what two independent
                   draws of num_samples / 2 from ONE distribution give.  A ``swd_split`` at or below it says nothing.  It does
                   not depend on the student and is repeated along that axis.

    The even and odd halves are strided views of the grids, read in place.  Returns numpy float64 arrays
    [student][scale][state] ``swd``, ``swd_split``, ``floor`` and ``max_swd``, ``argmax`` and ``status`` of the full
    comparison, ``states``, ``guidance_scales`` (NaN for None) and ``directions`` [L, E], and writes one
    ``swd_student_{k}.npz`` per student under ``output_dir`` (default ``config.analysis_dir``/sliced_wasserstein)."""
    from ..trajectory_engine import sample_grid
    from ...synthetic import noise_table
    from .perceptual import state_indices
    students, scales = list(student_models), list(guidance_scales)
    if not students or not scales:
        raise ValueError("sliced_wasserstein_sweep needs at least one student and one guidance scale")
    if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)) or num_samples < 2:
        raise ValueError(f"num_samples={num_samples!r} must be an int >= 2: the split needs an even and an odd sample")
    if num_samples > engine.SWD_MAX_N:
        raise ValueError(f"num_samples={num_samples} is above the {engine.SWD_MAX_N} rows a set may hold")
    derived_distances(0.0, 0.0, p)
    C, H, T, S = config.channels, config.image_size, config.timesteps, int(num_samples)
    for m in [teacher_model] + students:
        if getattr(m, "image_size", H) != H:
            raise ValueError("sliced_wasserstein_sweep compares states of one shape: every model needs the teacher's resolution")
    idx = state_indices(T + 1, every)
    host_directions = engine.swd_directions(C * H * H, n_directions, 0)
    device = next(teacher_model.parameters()).device
    if output_dir is None:
        output_dir = os.path.join(config.analysis_dir, "sliced_wasserstein")
    os.makedirs(output_dir, exist_ok=True)
    for m in [teacher_model] + students:
        m.eval()
    keys = ("swd", "swd_split", "floor", "max_swd", "argmax", "status")
    with torch.cuda.device(device):
        theta = host_directions.to(device)
        table = noise_table(42, S + T - 1, (1, C, H, H)).reshape(S + T - 1, -1).to(device)
        t_grid = sample_grid(engine.UNetHandle.for_module(teacher_model), table, 0, S, T, scales, H, H)
        teacher = []
        for gs in scales:
            tv = _state_view(t_grid[gs], idx)
            even = engine.device_swd_sorted(tv[:, 0::2], theta)
            floor = _distances(even, tv[:, 1::2], None, n_directions, p, 0)["swd"]
            teacher.append((engine.device_swd_sorted(tv, theta), even, floor))
        per_student = []
        for m in students:
            s_grid = sample_grid(engine.UNetHandle.for_module(m), table, 0, S, T, scales, H, H)
            cells = []
            for gs, (full, even, floor) in zip(scales, teacher):
                sv = _state_view(s_grid[gs], idx)
                cell = _distances(full, sv, None, n_directions, p, 0)
                cell["swd_split"] = _distances(even, sv[:, 1::2], None, n_directions, p, 0)["swd"]
                cell["floor"] = floor
                cells.append(cell)
            per_student.append({k: np.stack([c[k] for c in cells]) for k in keys})
    res = {k: np.stack([s[k] for s in per_student]) for k in keys}
    res.update(states=np.array(idx), guidance_scales=np.array([np.nan if gs is None else float(gs) for gs in scales]),
               directions=host_directions.numpy().copy())
    for k in range(len(students)):
        np.savez(os.path.join(output_dir, f"swd_student_{k}.npz"),
                 **{key: (res[key][k] if key in keys else res[key]) for key in res})
    return res
