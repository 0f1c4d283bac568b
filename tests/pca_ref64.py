"""float64 yardstick of the device PCA (include/dt_hip_pca.h): numpy SVD of the centred float64 rows, with the sign rule
of sklearn's svd_flip(u_based_decision=False) restated, so that it needs no sklearn.  Same quantities and names as
``sklearn.decomposition.PCA(n_components=k, svd_solver="full")``."""
import numpy as np


def pca_ref64(X, k):
    """dict(mean, components [k, E], scores [n, k], singular_values, explained_variance, explained_variance_ratio) of
    the rows X [n, E] (any dtype; computed on the float64 copy), and beyond the first k: spectrum [min(n, E)], every
    squared singular value (the eigenvalues of the centred Gram matrix, descending), and basis [min(n, E), E], every
    right singular vector with the sign rule applied."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    n = X.shape[0]
    mean = X.mean(axis=0)
    Xc = X - mean
    U, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    idx = np.argmax(np.abs(Vt), axis=1)                     # first index of the largest |entry| of each component
    signs = np.sign(Vt[np.arange(Vt.shape[0]), idx])
    U, Vt = U * signs, Vt * signs[:, None]
    var = S ** 2 / (n - 1)
    total = var.sum()
    return {"mean": mean, "components": Vt[:k], "scores": U[:, :k] * S[:k], "singular_values": S[:k],
            "explained_variance": var[:k], "explained_variance_ratio": var[:k] / total, "spectrum": S ** 2, "basis": Vt}


def ambiguous_sign(component, tol=1e-6):
    """True when the two largest |entries| of a component lie within ``tol`` of each other with opposite signs: then
    either sign is the right one up to rounding, and a comparison accepts both."""
    c = np.asarray(component, dtype=np.float64)
    order = np.argsort(-np.abs(c), kind="stable")
    if len(c) < 2:
        return False
    a, b = c[order[0]], c[order[1]]
    return abs(abs(a) - abs(b)) <= tol * abs(a) and np.sign(a) != np.sign(b)
