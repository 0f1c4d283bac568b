"""float64 yardstick of the device Fréchet distance (include/dt_hip_fid.h): the centred float64 copies of the two feature
sets and numpy's SVD of their cross product,

    tr sqrt(S_a S_b) = (sum of the singular values of A_c B_c^T) / sqrt((n_a - 1)(n_b - 1)).

It never calls the code under test.  tests/test_fid_host.py holds it against the committed ``calculate_fid`` (the
reference's np.cov / scipy sqrtm formula) where that one is well-posed."""
import numpy as np


def fid_ref64(a, b):
    """dict(fid, parts = (|mu_a - mu_b|^2, tr S_a, tr S_b, tr sqrt(S_a S_b)), scale = tr S_a + tr S_b) of the feature
    sets a [n_a, D], b [n_b, D] (any dtype; computed on the float64 copies)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n_a, n_b = len(a), len(b)
    mu_a, mu_b = a.mean(axis=0), b.mean(axis=0)
    ac, bc = a - mu_a, b - mu_b
    dmu2 = float(np.sum((mu_a - mu_b) ** 2))
    tr_a = float(np.sum(ac * ac) / (n_a - 1))
    tr_b = float(np.sum(bc * bc) / (n_b - 1))
    cross = float(np.linalg.svd(ac @ bc.T, compute_uv=False).sum() / np.sqrt((n_a - 1.0) * (n_b - 1.0)))
    return {"fid": dmu2 + tr_a + tr_b - 2.0 * cross, "parts": np.array([dmu2, tr_a, tr_b, cross]),
            "scale": tr_a + tr_b}


def feature_like(seed, n, D, rank=None, offset=0.4, spread=0.15, shift=0.0):
    """Seeded fp32 rows that look like pooled Inception features: a large common offset per column, a
    decaying spectrum.  ``rank``: the rows vary in a subspace of that dimension only (default: full)."""
    g = np.random.default_rng(seed)
    r = D if rank is None else rank
    basis = g.standard_normal((r, D)) / np.sqrt(r)
    coeff = g.standard_normal((n, r)) * (1.0 / np.sqrt(1.0 + np.arange(r)))
    base = offset * (1.0 + g.random(D)) + shift
    return (base + spread * (coeff @ basis)).astype(np.float32)
