"""Exact, deterministic PCA on the device (dt_pca_fit / dt_pca_project, include/dt_hip_pca.h).

The result is that of ``sklearn.decomposition.PCA(n_components=k, svd_solver="full")`` on the float64 copy of the fp32
rows: column mean, singular values, explained variance and ratio, components with svd_flip's sign rule, scores.  The
reference's callers run sklearn's default solver, which is randomized for these shapes and takes no random_state, so its
own numbers change from run to run (tests/test_pca_host.py records by how much).

Two places where the answer is not sklearn's vector for vector (include/dt_hip_pca.h): inside a repeated eigenvalue the
components are some orthonormal basis of the same subspace, and a direction without variance (a rank below
``n_components``) is reported as zeros (singular value, variances, component, scores) where sklearn returns an arbitrary
unit vector.
"""
import warnings

import numpy as np
import torch

from ... import engine

_ATTRS = ("singular_values", "explained_variance", "explained_variance_ratio")


def _device():
    if not torch.cuda.is_available():
        raise engine.HipLibraryError("TrajectoryPCA runs on the HIP device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _rows(X):
    """(device fp32 [n, E] rows, kind) for a numpy array or a tensor with one row per state (each row flattened)."""
    if isinstance(X, np.ndarray):
        t, kind = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)), "numpy"
    elif isinstance(X, torch.Tensor):
        t, kind = X.detach(), X.device
    else:
        raise ValueError(f"expected a numpy array or a torch tensor, got {type(X).__name__}")
    if t.dim() < 2:
        raise ValueError(f"expected one row per state (at least 2-D), got shape {tuple(t.shape)}")
    return t.reshape(t.shape[0], -1).float(), kind


def _out(t, kind):
    return t.cpu().numpy() if kind == "numpy" else t.to(kind)


class TrajectoryPCA:
    """sklearn-style PCA of the rows of one matrix, fitted on the device.  Attributes after ``fit`` are numpy arrays with
    sklearn's names; ``transform`` and ``fit_transform`` return numpy for numpy input and a tensor on the input's device
    for tensor input."""

    def __init__(self, n_components=2):
        self.n_components = n_components

    def _fit(self, X):
        rows, kind = _rows(X)
        engine._pca_check(rows, None, self.n_components)          # argument errors before any device work
        rows = rows if rows.is_cuda else rows.to(_device())
        r = engine.device_pca(rows, self.n_components)
        status = int(r["status"][0].item())
        if status == 1:
            raise ValueError("Input X contains NaN or infinity.")
        if status == 2:
            warnings.warn("TrajectoryPCA: the rows have zero total variance; explained_variance_ratio_ is NaN",
                          RuntimeWarning)
        self._mean_dev, self._comp_dev = r["mean"][0], r["components"][0]
        self.mean_ = self._mean_dev.cpu().numpy()
        self.components_ = self._comp_dev.cpu().numpy()
        for name in _ATTRS:
            setattr(self, name + "_", r[name][0].cpu().numpy())
        self.n_components_ = int(self.n_components)
        self.n_samples_, self.n_features_in_ = rows.shape
        return r["scores"][0], kind

    def fit(self, X, y=None):
        self._fit(X)
        return self

    def fit_transform(self, X, y=None):
        scores, kind = self._fit(X)
        return _out(scores, kind)

    def transform(self, X):
        if not hasattr(self, "_comp_dev"):
            raise ValueError("TrajectoryPCA is not fitted yet; call fit first")
        rows, kind = _rows(X)
        if rows.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {rows.shape[1]} features, but TrajectoryPCA was fitted with {self.n_features_in_}")
        scores = engine.device_pca_project(rows.to(self._comp_dev.device), self._mean_dev, self._comp_dev)[0]
        return _out(scores, kind)


def pca_pairs(X, Y, n_components):
    """Joint PCA of every sample pair of two step-major device trajectories X [nX, S, ...] and Y [nY, S, ...] in one call:
    problem s has the rows X[:, s] then Y[:, s].  Returns engine.device_pca's dict of device tensors ([S, ...])."""
    X = X.reshape(X.shape[0], X.shape[1], -1) if X.dim() != 3 else X
    Y = Y.reshape(Y.shape[0], Y.shape[1], -1) if Y.dim() != 3 else Y
    return engine.device_pca(X, n_components, Y)


def pca_sweep(teacher_model, student_models, config, guidance_scales, num_samples, n_components=2):
    """Joint teacher/student PCA of EVERY sample of a grid cell: ``sample_grid`` for each model (sample s starts from
    seed 42 + s, as the grid does), then ``pca_pairs`` for each (student, scale).  Returns numpy arrays indexed
    [i_student][i_scale][sample]: mean [.., E], components [.., k, E], scores [.., nT + nS, k], singular_values,
    explained_variance, explained_variance_ratio [.., k], status [..]; only these results leave the device."""
    from ..trajectory_engine import sample_grid
    from ...synthetic import noise_table
    device = next(teacher_model.parameters()).device
    C, H, T, S = config.channels, config.image_size, config.timesteps, num_samples
    scales = list(guidance_scales)
    with torch.cuda.device(device):
        table = noise_table(42, S + T - 1, (1, C, H, H)).reshape(S + T - 1, -1).to(device)
        t_grid = sample_grid(engine.UNetHandle.for_module(teacher_model), table, 0, S, T, scales, H, H)
        per_student = []
        for m in student_models:
            s_grid = sample_grid(engine.UNetHandle.for_module(m), table, 0, S, T, scales, H, H)
            per_student.append([pca_pairs(t_grid[gs], s_grid[gs], n_components) for gs in scales])
    keys = ("mean", "components", "scores") + _ATTRS + ("status",)
    return {key: torch.stack([torch.stack([r[key] for r in row]) for row in per_student]).cpu().numpy() for key in keys}
