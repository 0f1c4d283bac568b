"""The yardstick for trajectory alignment (include/dt_hip_align.h), in plain numpy and Python loops.

``cost_matrix``: differences in float64, their squares summed over E in np.longdouble and rounded once, then the square
root.  ``dp``: the recurrences, the tie order and the band rule of the header, cell by cell, and the walk back along the
chosen predecessors.  ``brute_force`` enumerates every monotone path (tiny shapes only)."""
import math

import numpy as np

DTW, FRECHET = "dtw", "frechet"
OK, NONFINITE, NO_PATH = 0, 1, 2


def cost_matrix(a, b):
    """[n_a, n_b] float64 of ||a_i - b_j||_2 for float32 rows a [n_a, E], b [n_b, E]"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
    for i in range(a.shape[0]):
        d = (a[i][None, :] - b).astype(np.longdouble)
        out[i] = np.sqrt((d * d).sum(axis=1)).astype(np.float64)
    return out


def band_mask(n_a, n_b, band):
    """allowed[i, j] of the integer band rule; band == 0: everything"""
    if band == 0:
        return np.ones((n_a, n_b), dtype=bool)
    i = np.arange(n_a, dtype=np.int64)[:, None]
    j = np.arange(n_b, dtype=np.int64)[None, :]
    return np.abs(i * (n_b - 1) - j * (n_a - 1)) <= band * max(n_a - 1, n_b - 1)


def dp(D, kind, band=0, allowed=None):
    """(value, path [L, 2] int32, status) of one float64 matrix D.  ``allowed`` overrides the band's mask.  NONFINITE: value
    NaN, empty path; NO_PATH: value +inf, empty path."""
    D = np.asarray(D, dtype=np.float64)
    n_a, n_b = D.shape
    empty = np.zeros((0, 2), dtype=np.int32)
    if not np.isfinite(D).all():
        return float("nan"), empty, NONFINITE
    if allowed is None:
        allowed = band_mask(n_a, n_b, band)
    # Python floats are IEEE doubles: lists of them keep the loops quick at 1024 x 1024
    Dl, ok = D.tolist(), np.asarray(allowed, dtype=bool).tolist()
    C = [[math.inf] * n_b for _ in range(n_a)]
    pred = [[3] * n_b for _ in range(n_a)]
    for i in range(n_a):
        for j in range(n_b):
            if not ok[i][j]:
                continue
            if i == 0 and j == 0:
                C[0][0] = Dl[0][0]
                continue
            m, code = None, 3
            if i > 0 and j > 0:
                m, code = C[i - 1][j - 1], 0
            if i > 0 and (m is None or C[i - 1][j] < m):
                m, code = C[i - 1][j], 1
            if j > 0 and (m is None or C[i][j - 1] < m):
                m, code = C[i][j - 1], 2
            C[i][j] = m + Dl[i][j] if kind == DTW else max(Dl[i][j], m)
            pred[i][j] = code
    value = C[n_a - 1][n_b - 1]
    if math.isinf(value):
        return value, empty, NO_PATH
    i, j, rev = n_a - 1, n_b - 1, []
    while True:
        rev.append((i, j))
        if i == 0 and j == 0:
            break
        code = pred[i][j]
        i, j = (i - 1, j - 1) if code == 0 else (i - 1, j) if code == 1 else (i, j - 1)
    return value, np.array(rev[::-1], dtype=np.int32), OK


def monotone_paths(n_a, n_b):
    """every path from (0, 0) to (n_a-1, n_b-1) with steps (1, 1), (1, 0), (0, 1)"""
    def walk(i, j):
        if i == n_a - 1 and j == n_b - 1:
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < n_a and j + dj < n_b:
                for rest in walk(i + di, j + dj):
                    yield [(i, j)] + rest
    return walk(0, 0)


def brute_force(D, kind):
    """the least path cost over every monotone path: math.fsum of the cells (DTW) or their maximum (Frechet)"""
    D = np.asarray(D, dtype=np.float64)
    best = math.inf
    for path in monotone_paths(*D.shape):
        cells = [float(D[i, j]) for i, j in path]
        best = min(best, math.fsum(cells) if kind == DTW else max(cells))
    return best


def path_value(D, path, kind):
    cells = [float(D[i, j]) for i, j in path]
    return math.fsum(cells) if kind == DTW else max(cells)


def align(a, b, kind, band=0):
    """(value, path, status, cost) from the rows"""
    D = cost_matrix(a, b)
    return dp(D, kind, band) + (D,)
