"""How far is the student's DISTRIBUTION of states from the teacher's at a reverse step, measured in the full state space?
The debiased Sinkhorn divergence (Feydy et al. 2019) between the set of the teacher's states and the set of the student's
states at a step,

    S_eps(A, B) = OT_eps(A, B) - 1/2 OT_eps(A, A) - 1/2 OT_eps(B, B),

with OT_eps the entropic optimal-transport cost (engine.device_sinkhorn_ot: csrc/dt_sinkhorn.hip).  The sliced Wasserstein
distance (sliced_wasserstein.py) sees the two sets through 1-D projections only; this couples them in R^E: it is zero
exactly when the sets coincide, needs no network and no weights, works at every step and on sets of unequal size, and moves
from W_p^p (small eps) to an MMD (large eps).  Beyond the reference, which has no such stage; no figures.

epsilon.  ``epsilon=None`` means ``rel_epsilon`` times the mean self cost of the TEACHER's set at that state, made on the
device (engine.device_sinkhorn_mean_cost).  Taking it from the teacher alone lets the three terms of a divergence share one
epsilon, and lets the teacher's self term be computed once and shared by every student.  The smaller epsilon, the more steps:
at rel_epsilon = 0.05 Gaussian sets of 64 rows take tens to a few hundred steps to a marginal error of 1e-10, at 0.01 tens of
thousands.  A student that follows the teacher sample by sample to within a fraction of epsilon (the paired comparison of
a good student) makes the plan a near-permutation: the potentials of the samples are then coupled through exp(-gap / epsilon)
only, and the marginal error stays near n exp(-gap / epsilon) -- 5e-8 for 256 Gaussian rows of 768 and a student at 0.1 of
the teacher's spread -- for millions of steps, although the value has long settled.  Hence the default ``tol`` of 1e-6 on the
L1 marginal error.  A state that has not reached ``tol`` within ``max_iter`` steps is flagged (status bit 4) and its value
still given; nothing is promised for small epsilon."""
import os

import numpy as np
import torch

from ... import engine
from .spectral import _state_view
from .trajectory_metrics import _prepare

DEFAULT_REL_EPSILON = 0.05


def relative_epsilon(mean_cost, rel_epsilon):
    """epsilon = rel_epsilon * mean_cost in float64: a tensor stays on its device; rel_epsilon must be positive and finite"""
    if isinstance(rel_epsilon, bool) or not isinstance(rel_epsilon, (int, float, np.integer, np.floating)) \
            or not (np.isfinite(rel_epsilon) and rel_epsilon > 0):
        raise ValueError(f"rel_epsilon={rel_epsilon!r} must be a positive finite float")
    if isinstance(mean_cost, torch.Tensor):
        return mean_cost.to(torch.float64) * float(rel_epsilon)
    return np.asarray(mean_cost, dtype=np.float64) * np.float64(rel_epsilon)


def teacher_epsilon(X, epsilon, rel_epsilon, p):
    """the epsilon of a comparison against the teacher's states X: ``epsilon`` where given (a float), else the float64 device
    tensor rel_epsilon * mean self cost of X, one value per state"""
    relative_epsilon(0.0, rel_epsilon)
    if epsilon is not None:
        return epsilon
    return relative_epsilon(engine.device_sinkhorn_mean_cost(X, X, p=p)["mean_cost"], rel_epsilon)


def _numpy(out, eps, P):
    res = {k: out[k].cpu().numpy() for k in ("divergence", "err", "iters", "status")}
    res["ot"] = np.stack([out[k].cpu().numpy() for k in ("ot_ab", "ot_aa", "ot_bb")], axis=-1)
    res["epsilon"] = eps.cpu().numpy() if isinstance(eps, torch.Tensor) else np.full(P, float(eps))
    return res


def sinkhorn_pairs(X, Y, epsilon=None, rel_epsilon=DEFAULT_REL_EPSILON, p=2, max_iter=engine.SINKHORN_DEFAULT_MAX_ITER,
                   tol=engine.SINKHORN_DEFAULT_TOL, self_x=None):
    """Sinkhorn divergence between the sets of X (teacher) and of Y (student), state by state: device tensors [n, S, E]
    float32 (state i holds a set of S rows; views are read in place; the set sizes of X and Y may differ; [S, E] is one
    state).  ``engine.device_sinkhorn_divergence`` with one epsilon per state (see the module docstring).  ``self_x``: the
    teacher's self term made earlier with the same epsilon.  Returns numpy arrays ``divergence`` [n] float64, ``ot`` [n, 3]
    (OT_eps(X, Y), OT_eps(X, X), OT_eps(Y, Y)), ``epsilon`` [n], ``err`` [n] and ``iters`` [n] (the largest of the three
    problems), ``status`` [n] (their bits OR-ed: 1 a NaN or Inf in the state, 2 an epsilon that is not positive -- a
    teacher set of one row has none --, 4 not converged within max_iter)."""
    eps = teacher_epsilon(X, epsilon, rel_epsilon, p)
    out = engine.device_sinkhorn_divergence(X, Y, eps, p=p, max_iter=max_iter, tol=tol, self_a=self_x)
    return _numpy(out, eps, out["divergence"].shape[0])


def sinkhorn_trajectories(teacher_trajectory, student_trajectory, epsilon=None, rel_epsilon=DEFAULT_REL_EPSILON, p=2,
                          max_iter=engine.SINKHORN_DEFAULT_MAX_ITER, tol=engine.SINKHORN_DEFAULT_TOL):
    """The same for one (teacher, student) pair in the reference's trajectory forms (lists of tensors [B, C, H, W] or of
    (tensor, t) tuples, as ``align_trajectories`` takes them; a student of another resolution is resized to the
    teacher's).  State i of the teacher meets state i of the student: the lengths must be equal.  The B pictures of an
    entry are its set; the student's B may differ from the teacher's."""
    if len(teacher_trajectory) != len(student_trajectory):
        raise ValueError(f"the teacher has {len(teacher_trajectory)} states, the student {len(student_trajectory)}: "
                         "the divergence pairs them one to one")
    X, Y, device = _prepare(teacher_trajectory, student_trajectory)
    for images in (X, Y):
        if images[0].dim() != 4 or any(x.shape != images[0].shape for x in images):
            raise ValueError("every state of a trajectory must be a tensor [B, C, H, W] of one shape")
    if X[0].shape[1:] != Y[0].shape[1:]:
        raise ValueError(f"teacher states are {tuple(X[0].shape[1:])}, student states {tuple(Y[0].shape[1:])}")
    stack = lambda images: torch.stack([im.detach().reshape(im.shape[0], -1) for im in images]).to(device=device, dtype=torch.float32)
    return sinkhorn_pairs(stack(X), stack(Y), epsilon, rel_epsilon, p, max_iter, tol)


def sinkhorn_sweep(teacher_model, student_models, config, guidance_scales, num_samples, every=1, epsilon=None,
                   rel_epsilon=DEFAULT_REL_EPSILON, p=2, max_iter=engine.SINKHORN_DEFAULT_MAX_ITER,
                   tol=engine.SINKHORN_DEFAULT_TOL, output_dir=None):
    """Sinkhorn divergences of every student against one teacher, for every guidance scale and state.  The trajectories
    come from ``sample_grid`` exactly as ``sliced_wasserstein_sweep`` runs it (``noise_table(42, ...)``, sample s from seed
    42 + s); the teacher is sampled once for all scales, every ``every``-th state plus the last is taken
    (``perceptual.state_indices``).  epsilon comes from the teacher's sets alone (module docstring), so the teacher's self
    terms are made once per scale and shared by all students.  Per (student, scale, state), as in the sliced sweep:

    ``divergence``        all of the teacher's samples against all of the student's: a PAIRED comparison (sample s of both
                          starts from the same seed), exactly 0 for a student that reproduces the teacher.
    ``divergence_split``  the teacher's even-numbered samples against the student's odd-numbered ones: two independent
                          draws.  This is the number to hold against ``floor``.
    ``floor``             the teacher's even-numbered samples against its own odd-numbered ones; it does not depend on the
                          student and is repeated along that axis.

    The split terms use the epsilon of the teacher's even half.  Returns numpy arrays [student][scale][state]
    ``divergence``, ``divergence_split``, ``floor``, and of the full comparison ``ot`` [.., 3], ``epsilon``, ``err``,
    ``iters``, ``status``; ``states``, ``guidance_scales`` (NaN for None); and writes one ``sinkhorn_student_{k}.npz`` per
    student under ``output_dir`` (default ``config.analysis_dir``/sinkhorn)."""
    from ..trajectory_engine import sample_grid
    from ...synthetic import noise_table
    from .perceptual import state_indices
    students, scales = list(student_models), list(guidance_scales)
    if not students or not scales:
        raise ValueError("sinkhorn_sweep needs at least one student and one guidance scale")
    if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)) or num_samples < 4:
        raise ValueError(f"num_samples={num_samples!r} must be an int >= 4: each half of the split needs two samples for its epsilon")
    if num_samples > engine.SINKHORN_MAX_N:
        raise ValueError(f"num_samples={num_samples} is above the {engine.SINKHORN_MAX_N} rows a set may hold")
    engine._sinkhorn_p(p), engine._sinkhorn_stop(max_iter, tol), relative_epsilon(0.0, rel_epsilon)
    if epsilon is not None:
        engine._sinkhorn_epsilon(epsilon, 1)
    C, H, T, S = config.channels, config.image_size, config.timesteps, int(num_samples)
    for m in [teacher_model] + students:
        if getattr(m, "image_size", H) != H:
            raise ValueError("sinkhorn_sweep compares states of one shape: every model needs the teacher's resolution")
    idx = state_indices(T + 1, every)
    device = next(teacher_model.parameters()).device
    if output_dir is None:
        output_dir = os.path.join(config.analysis_dir, "sinkhorn")
    os.makedirs(output_dir, exist_ok=True)
    for m in [teacher_model] + students:
        m.eval()
    kw = dict(p=p, max_iter=max_iter, tol=tol)
    keys = ("divergence", "divergence_split", "floor", "ot", "epsilon", "err", "iters", "status")
    with torch.cuda.device(device):
        table = noise_table(42, S + T - 1, (1, C, H, H)).reshape(S + T - 1, -1).to(device)
        t_grid = sample_grid(engine.UNetHandle.for_module(teacher_model), table, 0, S, T, scales, H, H)
        teacher = []
        for gs in scales:
            tv = _state_view(t_grid[gs], idx)
            even, odd = tv[:, 0::2], tv[:, 1::2]
            eps, eps_even = teacher_epsilon(tv, epsilon, rel_epsilon, p), teacher_epsilon(even, epsilon, rel_epsilon, p)
            full_self = engine.device_sinkhorn_ot(tv, tv, eps, **kw)
            even_self = engine.device_sinkhorn_ot(even, even, eps_even, **kw)
            floor = engine.device_sinkhorn_divergence(even, odd, eps_even, self_a=even_self, **kw)["divergence"].cpu().numpy()
            teacher.append((tv, even, eps, eps_even, full_self, even_self, floor))
        per_student = []
        for m in students:
            s_grid = sample_grid(engine.UNetHandle.for_module(m), table, 0, S, T, scales, H, H)
            cells = []
            for gs, (tv, even, eps, eps_even, full_self, even_self, floor) in zip(scales, teacher):
                sv = _state_view(s_grid[gs], idx)
                cell = _numpy(engine.device_sinkhorn_divergence(tv, sv, eps, self_a=full_self, **kw), eps, len(idx))
                split = engine.device_sinkhorn_divergence(even, sv[:, 1::2], eps_even, self_a=even_self, **kw)
                cell["divergence_split"] = split["divergence"].cpu().numpy()
                cell["floor"] = floor
                cells.append(cell)
            per_student.append({k: np.stack([c[k] for c in cells]) for k in keys})
    res = {k: np.stack([s[k] for s in per_student]) for k in keys}
    res.update(states=np.array(idx), guidance_scales=np.array([np.nan if gs is None else float(gs) for gs in scales]))
    for k in range(len(students)):
        np.savez(os.path.join(output_dir, f"sinkhorn_student_{k}.npz"),
                 **{key: (res[key][k] if key in keys else res[key]) for key in res})
    return res
