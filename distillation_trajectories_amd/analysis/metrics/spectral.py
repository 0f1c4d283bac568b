"""Which spatial scales does a student get wrong, and at which step does that start?  The per-band power spectrum of the
teacher's and the student's states and the per-band cross-spectrum between them (engine.device_spectral_pair:
csrc/dt_spectral.hip), band by band of a radial binning of the 2-D DFT of every channel.

A reverse trajectory builds a picture from coarse to fine; the MSE between two states is one number and mixes a wrong
layout (an error at low frequencies, early) with lost texture (an error at high frequencies, late).  ``relative_error``
per band and step separates the two, ``band_correlation`` says whether a band's content is misplaced or merely weaker, and
``log_spectral_distance`` is the usual one-number summary of the two power spectra.  Beyond the reference, which has no
spectral stage; no figures."""
import os

import numpy as np
import torch

from ... import engine
from .trajectory_metrics import _prepare


def derived_metrics(power_a, power_b, cross_re, error, count, cells_per_bin, C, H, W):
    """The band metrics from sample-and-channel sums [states, bins] (float64 or wider), ``count`` [states] and
    ``cells_per_bin`` [bins]: ``power_teacher`` and ``power_student`` (mean per coefficient: sum / (count C cells H W)),
    ``band_correlation`` = C_re / sqrt(P_a P_b), ``relative_error`` = D / P_a and ``log_spectral_distance`` [states] =
    sqrt(mean over bins of (10 log10(power_student / power_teacher))^2).  A bin with P_a == 0 gives NaN in the two ratios
    and is left out of the log distance (all bins left out: NaN); an empty bin has NaN power."""
    dtype = np.result_type(power_a.dtype, np.float64)
    norm = (np.asarray(count, dtype=dtype)[:, None] * (C * H * W)) * np.asarray(cells_per_bin, dtype=dtype)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        has = power_a > 0
        res = {"power_teacher": power_a / norm, "power_student": power_b / norm,
               "band_correlation": np.where(has, cross_re / np.sqrt(power_a * power_b), np.nan),
               "relative_error": np.where(has, error / power_a, np.nan)}
        db = np.where(has, 10.0 * np.log10(power_b / np.where(has, power_a, 1)), 0) ** 2
        n = has.sum(axis=1)
        res["log_spectral_distance"] = np.where(n > 0, np.sqrt(db.sum(axis=1) / np.maximum(n, 1)), np.nan)
    return res


def spectral_pairs(X, Y, C, H, W):
    """Band metrics of device trajectories X (teacher) and Y (student), [n, S, E] float32 with E = C*H*W in NCHW order
    (views are read in place; [Q, E] is one state of Q samples): ONE ``engine.device_spectral_pair`` call that also sums
    over the samples, then numpy float64 on the sums, channels added.  Returns ``derived_metrics`` [n, n_bins] (and
    ``log_spectral_distance`` [n]) together with ``count`` [n] (the samples behind a state: those without a NaN or Inf),
    ``status`` [n, S], ``radius`` [n_bins] (the bin index: cycles per picture) and ``cells_per_bin``."""
    if isinstance(X, torch.Tensor) and isinstance(Y, torch.Tensor) and X.dim() == 2 and Y.dim() == 2:
        X, Y = X.unsqueeze(0), Y.unsqueeze(0)
    out = engine.device_spectral_pair(X, Y, C, H, W, sum_samples=True)
    _, cells = engine.radial_bins(H, W)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    chan = lambda a: a.sum(axis=1)
    res = derived_metrics(chan(host["power_a"]), chan(host["power_b"]), chan(host["cross"][..., 0]), chan(host["error"]),
                          host["count"], cells, C, H, W)
    res.update(count=host["count"], status=host["status"], radius=np.arange(len(cells)), cells_per_bin=cells)
    return res


def spectral_trajectories(teacher_trajectory, student_trajectory):
    """The same for one (teacher, student) pair in the reference's trajectory forms (lists of tensors [B, C, H, W] or of
    (tensor, t) tuples, as ``align_trajectories`` takes them; a student of another resolution is resized to the
    teacher's).  State i of the teacher meets state i of the student: the lengths must be equal.  The B pictures of an
    entry are its samples."""
    X, Y, device = _prepare(teacher_trajectory, student_trajectory)
    if len(X) != len(Y):
        raise ValueError(f"the teacher has {len(X)} states, the student {len(Y)}: a spectral comparison pairs them one to one")
    if X[0].dim() != 4 or any(x.shape != X[0].shape for x in X) or any(y.shape != X[0].shape for y in Y):
        raise ValueError("every state must be a tensor [B, C, H, W] of one shape")
    B, C, H, W = X[0].shape
    stack = lambda images: torch.stack([im.detach().reshape(B, -1) for im in images]).to(device=device, dtype=torch.float32)
    return spectral_pairs(stack(X), stack(Y), C, H, W)


def _state_view(states, idx):
    """the states ``idx`` of a trajectory tensor: a strided view where the indices are evenly spaced, a gather otherwise"""
    if len(idx) == 1:
        return states[idx[0]:idx[0] + 1]
    step = idx[1] - idx[0]
    if all(b - a == step for a, b in zip(idx, idx[1:])):
        return states[idx[0]:idx[-1] + 1:step]
    return states[idx]


def spectral_sweep(teacher_model, student_models, config, guidance_scales, num_samples, every=1, output_dir=None):
    """Band metrics of every student against one teacher, for every guidance scale.  The trajectories come from
    ``sample_grid`` exactly as ``pca_sweep``, ``lpips_sweep`` and ``cka_sweep`` run it (``noise_table(42, ...)``, sample s
    from seed 42 + s); the teacher is sampled once for all scales, every ``every``-th state plus the last is taken
    (``perceptual.state_indices``), and each (student, scale) is ONE ``engine.device_spectral_pair`` call on views of the
    grids.  Returns numpy arrays indexed [student][scale][state][bin] (``power_teacher``, ``power_student``,
    ``band_correlation``, ``relative_error``), ``log_spectral_distance`` [student][scale][state], ``count``
    [student][scale][state], ``status`` [student][scale][state][sample], ``states``, ``guidance_scales`` (NaN for None),
    ``radius`` and ``cells_per_bin``, and writes one ``spectral_student_{k}.npz`` per student under ``output_dir``
    (default ``config.analysis_dir``/spectral)."""
    from ..trajectory_engine import sample_grid
    from ...synthetic import noise_table
    from .perceptual import state_indices
    students, scales = list(student_models), list(guidance_scales)
    if not students or not scales:
        raise ValueError("spectral_sweep needs at least one student and one guidance scale")
    if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)) or num_samples < 1:
        raise ValueError(f"num_samples={num_samples!r} must be an int >= 1")
    C, H, T, S = config.channels, config.image_size, config.timesteps, int(num_samples)
    engine.radial_bins(H, H)                      # the limits of a spectrum, before anything is sampled
    if not 1 <= C <= engine.SPECTRAL_MAX_C:
        raise ValueError(f"a spectrum takes 1 <= C <= {engine.SPECTRAL_MAX_C} channels, got {C}")
    for m in [teacher_model] + students:
        if getattr(m, "image_size", H) != H:
            raise ValueError("spectral_sweep pairs states pixel by pixel: every model needs the teacher's resolution")
    idx = state_indices(T + 1, every)
    device = next(teacher_model.parameters()).device
    if output_dir is None:
        output_dir = os.path.join(config.analysis_dir, "spectral")
    os.makedirs(output_dir, exist_ok=True)
    for m in [teacher_model] + students:
        m.eval()
    keys = ("power_teacher", "power_student", "band_correlation", "relative_error", "log_spectral_distance", "count", "status")
    with torch.cuda.device(device):
        table = noise_table(42, S + T - 1, (1, C, H, H)).reshape(S + T - 1, -1).to(device)
        t_grid = sample_grid(engine.UNetHandle.for_module(teacher_model), table, 0, S, T, scales, H, H)
        per_student = []
        for m in students:
            s_grid = sample_grid(engine.UNetHandle.for_module(m), table, 0, S, T, scales, H, H)
            cells = [spectral_pairs(_state_view(t_grid[gs], idx), _state_view(s_grid[gs], idx), C, H, H) for gs in scales]
            per_student.append({k: np.stack([c[k] for c in cells]) for k in keys})
    res = {k: np.stack([p[k] for p in per_student]) for k in keys}
    _, cells_per_bin = engine.radial_bins(H, H)
    res.update(states=np.array(idx), guidance_scales=np.array([np.nan if gs is None else float(gs) for gs in scales]),
               radius=np.arange(len(cells_per_bin)), cells_per_bin=cells_per_bin)
    for k in range(len(students)):
        np.savez(os.path.join(output_dir, f"spectral_student_{k}.npz"),
                 **{key: (res[key][k] if key in keys else res[key]) for key in res})
    return res
