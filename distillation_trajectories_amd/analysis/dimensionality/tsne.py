"""Exact t-SNE on the device (dt_tsne_affinities / dt_tsne_descend, include/dt_hip_tsne.h).

From a given start the method is deterministic: sklearn's ``TSNE(method="exact")`` with 2 components, the joint
probabilities from float64 distances, every step of the two-stage gradient descent in float64.  The optimiser is
chaotic (a rounding-size change of the start moves the final embedding by a good part of its extent), so runs are
compared by their KL divergence, not point by point.
"""
import numpy as np
import torch

from ... import engine
from .pca import _device, _rows


class TrajectoryTSNE:
    """sklearn-style t-SNE of the rows of one matrix (4 to 512 rows), fitted on the device.

    The method is sklearn's ``method="exact"``: the full n x n joint probabilities and the exact gradient of the KL
    divergence.  The reference's call, ``TSNE(n_components=2, perplexity=..., random_state=42)``, takes sklearn's default
    ``method="barnes_hut"``, an approximation of the same objective (nearest-neighbour affinities, a quad tree for the
    repulsive forces); its embedding is another local optimum of that objective, not this one point for point.

    ``init``: "pca" (the first two scores of the exact device PCA, divided by the standard deviation of the first and
    multiplied by 1e-4: sklearn's rule, with its randomized PCA replaced by the exact one), "random"
    (``1e-4 * RandomState(random_state).standard_normal((n, 2))`` as float32) or an array [n, 2].
    ``learning_rate="auto"`` is ``max(n / early_exaggeration / 4, 50)``.  After ``fit``: ``embedding_`` [n, 2] fp32,
    ``kl_divergence_`` (of that embedding), ``n_iter_`` (iterations done), ``learning_rate_``."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, init="pca", random_state=None):
        self.n_components = n_components
        self.perplexity = perplexity
        self.early_exaggeration = early_exaggeration
        self.learning_rate = learning_rate
        self.max_iter = max_iter
        self.n_iter_without_progress = n_iter_without_progress
        self.min_grad_norm = min_grad_norm
        self.init = init
        self.random_state = random_state

    def _start(self, rows):
        """the embedding before any iteration, [n, 2]"""
        n = rows.shape[0]
        if isinstance(self.init, (np.ndarray, torch.Tensor)):
            return self.init
        if self.init == "random":
            rng = self.random_state if isinstance(self.random_state, np.random.RandomState) \
                else np.random.RandomState(self.random_state)
            return 1e-4 * rng.standard_normal(size=(n, 2)).astype(np.float32)
        scores = engine.device_pca(rows, 2)["scores"][0].cpu().numpy()            # fp32, as sklearn's astype(float32)
        return scores / np.std(scores[:, 0]) * 1e-4

    def _kwargs(self):
        return dict(perplexity=self.perplexity, max_iter=self.max_iter, early_exaggeration=self.early_exaggeration,
                    learning_rate=self.learning_rate, n_iter_without_progress=self.n_iter_without_progress,
                    min_grad_norm=self.min_grad_norm)

    def _fit(self, X):
        if isinstance(self.n_components, bool) or self.n_components != 2:
            raise ValueError(f"n_components={self.n_components!r}: the device t-SNE embeds in 2 dimensions only")
        if not isinstance(self.init, (np.ndarray, torch.Tensor)) and self.init not in ("pca", "random"):
            raise ValueError(f"init={self.init!r} must be 'pca', 'random' or an array [n, 2]")
        rows, kind = _rows(X)
        n = rows.shape[0]
        probe = self.init if isinstance(self.init, (np.ndarray, torch.Tensor)) else np.zeros((n, 2), np.float32)
        engine._tsne_check(rows, None, self.perplexity, probe, self.max_iter, 0, None, None, self.early_exaggeration,
                           self.learning_rate, self.n_iter_without_progress, self.min_grad_norm, 250, (0.5, 0.8), 0.01,
                           50)                              # argument errors before any device work
        rows = rows if rows.is_cuda else rows.to(_device())
        self.init_embedding_ = self._start(rows)
        r = engine.device_tsne(rows, init=self.init_embedding_, **self._kwargs())
        if int(r["status"][0].item()) == 1:
            raise ValueError("Input X contains NaN or infinity.")
        self.embedding_ = r["embedding"][0].cpu().numpy()
        self.kl_divergence_ = float(r["kl_divergence"][0].item())
        self.n_iter_ = int(r["n_iter"][0].item())
        self.learning_rate_ = (max(n / self.early_exaggeration / 4.0, 50.0) if self.learning_rate == "auto"
                               else float(self.learning_rate))
        self.n_samples_, self.n_features_in_ = rows.shape
        return r["embedding"][0], kind

    def fit(self, X, y=None):
        self._fit(X)
        return self

    def fit_transform(self, X, y=None):
        emb, kind = self._fit(X)
        return emb.cpu().numpy() if kind == "numpy" else emb.to(kind)


def tsne_pairs(X, Y, perplexity, init, **kwargs):
    """Joint t-SNE of every sample pair of two step-major device trajectories X [nX, S, ...] and Y [nY, S, ...] in one
    call: problem s has the rows X[:, s] then Y[:, s].  ``init`` is [nX + nY, 2] for every pair or [S, nX + nY, 2];
    ``kwargs`` and the returned dict of device tensors ([S, ...]) are engine.device_tsne's."""
    X = X.reshape(X.shape[0], X.shape[1], -1) if X.dim() != 3 else X
    Y = Y.reshape(Y.shape[0], Y.shape[1], -1) if Y.dim() != 3 else Y
    return engine.device_tsne(X, Y, perplexity=perplexity, init=init, **kwargs)


def pca_start(X, Y):
    """sklearn's init="pca" for every pair of X [nX, S, E], Y [nY, S, E]: [S, nX + nY, 2] float64 on the device"""
    scores = engine.device_pca(X, 2, Y)["scores"].double()
    return scores / scores[:, :, 0].std(dim=1, unbiased=False)[:, None, None] * 1e-4


def tsne_sweep(teacher_model, student_models, config, guidance_scales, num_samples, perplexity=None, init="pca",
               random_state=42, **kwargs):
    """Joint teacher/student t-SNE of EVERY sample of a grid cell: ``sample_grid`` for each model (sample s starts from
    seed 42 + s, as the grid does), then one ``tsne_pairs`` call for each (student, scale).  ``perplexity`` defaults to the
    reference's ``min(30, n // 5)``; ``init`` is "pca" (per pair, ``pca_start``), "random" (one
    ``RandomState(random_state)`` draw shared by every pair) or an array.  Returns numpy arrays indexed
    [i_student][i_scale][sample]: embedding [.., nT + nS, 2], kl_divergence, n_iter, status; only these leave the device."""
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
            row = []
            for gs in scales:
                X, Y = t_grid[gs], s_grid[gs]
                n = X.shape[0] + Y.shape[0]
                if isinstance(init, str) and init == "pca":
                    start = pca_start(X, Y)
                elif isinstance(init, str) and init == "random":
                    start = 1e-4 * np.random.RandomState(random_state).standard_normal(size=(n, 2)).astype(np.float32)
                else:
                    start = init
                row.append(tsne_pairs(X, Y, min(30, n // 5) if perplexity is None else perplexity, start, **kwargs))
            per_student.append(row)
    keys = ("embedding", "kl_divergence", "n_iter", "status")
    return {key: torch.stack([torch.stack([r[key] for r in row]) for row in per_student]).cpu().numpy() for key in keys}
