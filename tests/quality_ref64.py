"""float64 yardstick of the device sample-quality scores (include/dt_hip_quality.h): KID, the squared k-th
nearest-neighbour radii and the four counts of precision / recall / density / coverage, in numpy, from exactly the header's
definitions.  It never calls the code under test.

Squared distances: for sets of up to 300 rows the direct differences sum (x_k - y_k)^2; for larger sets the Gram identity
on rows centred by the pooled mean (centring removes the common offset the features sit on, so the cancellation of that
form stays far below the bound).  KID always uses the un-centred Gram matrices, as the definition does.

Bounds (u = 2^-53), derived, not measured:
  d2, squared radii : 2 (D + 4) u (|x|^2 + |y|^2), three length-D FMA-chain dot products and their combination; for a
                      radius the largest row norm of its set on both sides.  ``d2_bound`` below is the largest of these
                      over both sets, 4 (D + 4) u max |row|^2, and is the unit of the gaps.
  KID               : 4 (3 (D + 2) + n_a + n_b) u S_kappa, S_kappa = mean kappa_AA + mean kappa_BB + 2 mean kappa_AB.
Counts are compared exactly, which is legitimate where every comparison ``d2 < r2`` that is not an exact tie between
bitwise-equal rows is decided by a margin of at least 100 bounds: ``min_gap``."""
import functools

import numpy as np

from fid_ref64 import feature_like

U = 2.0 ** -53
DIRECT_MAX = 300
MODES = ("same", "shift", "collapse", "spread")


def feature_pair(seed, n_a, n_b, D, mode="same", p=0):
    """(A [n_a, D], B [n_b, D]) fp32: one ``feature_like`` pool split in two; B as it is ("same"), with 0.002 (p + 1)
    added ("shift"), or scaled about the pooled mean by 0.5 - 0.1 p ("collapse") / 1.3 + 0.2 p ("spread")."""
    pool = feature_like(seed, n_a + n_b, D)
    a, b = pool[:n_a], pool[n_a:].astype(np.float64)
    if mode == "shift":
        b = b + 0.002 * (p + 1)
    elif mode in ("collapse", "spread"):
        mean = pool.astype(np.float64).mean(axis=0)
        b = mean + (0.5 - 0.1 * p if mode == "collapse" else 1.3 + 0.2 * p) * (b - mean)
    elif mode != "same":
        raise ValueError(mode)
    return a, b.astype(np.float32)


def d2_direct(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.stack([((xi - y) ** 2).sum(axis=1) for xi in x])


def d2_gram(x, y, centre):
    x, y = np.asarray(x, np.float64) - centre, np.asarray(y, np.float64) - centre
    return np.maximum((x * x).sum(axis=1)[:, None] + (y * y).sum(axis=1)[None, :] - 2.0 * (x @ y.T), 0.0)


def _kappa_sum(x, y, D, off_diagonal):
    K = (x @ y.T / D + 1.0) ** 3
    if off_diagonal:
        K = K[~np.eye(len(x), dtype=bool)]
    return float(K.sum()), float(K.mean())


def kid_ref64(a, b):
    """(kid, S_kappa) of the full sets"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    D = a.shape[1]
    (saa, maa), (sbb, mbb), (sab, mab) = _kappa_sum(a, a, D, True), _kappa_sum(b, b, D, True), _kappa_sum(a, b, D, False)
    n_a, n_b = len(a), len(b)
    return saa / (n_a * (n_a - 1)) + sbb / (n_b * (n_b - 1)) - 2.0 * sab / (n_a * n_b), maa + mbb + 2.0 * mab


def kid_tolerance(n_a, n_b, D, s_kappa):
    return 4.0 * (3.0 * (D + 2) + n_a + n_b) * U * s_kappa


def quality_ref64(a, b, k, form=None):
    """dict(kid, s_kappa, kid_tol, radii_a, radii_b (squared), counts [4] int64 = (precision hits, recall hits, density
    pairs, coverage hits), d2_bound, min_gap: the smallest non-zero |d2 - r2| over all comparisons, ties: the number of
    exact zeros among them, selection_gap: the smallest distance of a row's (k+1)-th entry from its neighbours in sorted
    order; both gaps in units of d2_bound) of the feature sets a [n_a, D] (real), b [n_b, D] (generated).  ``form``:
    "direct" or "gram" (default: by size)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n_a, n_b, D = len(a), len(b), a.shape[1]
    if form is None:
        form = "direct" if max(n_a, n_b) <= DIRECT_MAX else "gram"
    if form == "direct":
        daa, dbb, dab = d2_direct(a, a), d2_direct(b, b), d2_direct(a, b)
    else:
        centre = np.concatenate([a, b]).mean(axis=0)
        daa, dbb, dab = d2_gram(a, a, centre), d2_gram(b, b, centre), d2_gram(a, b, centre)
        np.fill_diagonal(daa, 0.0)
        np.fill_diagonal(dbb, 0.0)
    saa, sbb = np.sort(daa, axis=1), np.sort(dbb, axis=1)
    ra, rb = saa[:, k], sbb[:, k]
    in_a, in_b = dab < ra[:, None], dab < rb[None, :]
    counts = np.array([in_a.any(axis=0).sum(), in_b.any(axis=1).sum(), in_a.sum(),
                       (dab.min(axis=1) < ra).sum()], dtype=np.int64)
    norm2 = max((a * a).sum(axis=1).max(), (b * b).sum(axis=1).max())
    bound = 4.0 * (D + 4) * U * norm2
    gaps = np.concatenate([np.abs(dab - ra[:, None]).ravel(), np.abs(dab - rb[None, :]).ravel()])
    ties = int((gaps == 0.0).sum())
    min_gap = float(gaps[gaps > 0.0].min() / bound) if ties < gaps.size else float("inf")
    sel = []
    for s in (saa, sbb):
        sel.append((s[:, k] - s[:, k - 1]).min())
        if k + 1 < s.shape[1]:
            sel.append((s[:, k + 1] - s[:, k]).min())
    kid, s_kappa = kid_ref64(a, b)
    return {"kid": kid, "s_kappa": s_kappa, "kid_tol": kid_tolerance(n_a, n_b, D, s_kappa), "radii_a": ra, "radii_b": rb,
            "counts": counts, "d2_bound": bound, "min_gap": min_gap, "ties": ties,
            "selection_gap": float(min(sel) / bound)}


def radius_bounds(a, b):
    """the bound on a squared radius of set a, and of set b: 4 (D + 4) u max |row|^2 of that set"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    D = a.shape[1]
    return tuple(4.0 * (D + 4) * U * (x * x).sum(axis=1).max() for x in (a, b))


# ---------------------------------------------------------------------- the cases of tests/test_hip_quality.py
# name -> (n_a, n_b, P, D, k); the teacher (set A) is shared by the P problems of a case
SHAPES = {
    "50x50": (50, 50, 1, 2048, 5),
    "50x50_P11_shared": (50, 50, 11, 2048, 5),
    "8x50_P3": (8, 50, 3, 2048, 3),
    "7x6_kmax": (7, 6, 1, 2048, 5),
    "300x257_P2": (300, 257, 2, 2048, 3),
    "D80_65x64_P2": (65, 64, 2, 80, 5),
    "D80_64x65_P2": (64, 65, 2, 80, 5),
    "D36_129x63": (129, 63, 1, 36, 3),
    "2048x2048": (2048, 2048, 1, 2048, 5),
    "50x50_k1": (50, 50, 1, 2048, 1),
}
# the seed of a case's pool is 7000 + 13 n_a + n_b + D, except where that pool decides a comparison by little more than
# the 100 bounds the tests ask for (300 x 257: 102)
SEEDS = {"300x257_P2": 7002}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(a, [b_0 .. b_P-1], k, [quality_ref64 of (a, b_p)]) of a case: problem 0 is the pooled pair as it is, the others
    go through "shift", "collapse" and "spread" in turn with parameter (p - 1) // 3"""
    n_a, n_b, P, D, k = SHAPES[name]
    seed = SEEDS.get(name, 7000 + 13 * n_a + n_b + D)
    pairs = [feature_pair(seed, n_a, n_b, D, MODES[0 if p == 0 else 1 + (p - 1) % 3], 0 if p == 0 else (p - 1) // 3)
             for p in range(P)]
    a = pairs[0][0]
    assert all(np.array_equal(a, x) for x, _ in pairs)
    bs = [y for _, y in pairs]
    return a, bs, k, [quality_ref64(a, y, k) for y in bs]


# name -> k; the degenerate inputs of tests/test_hip_quality.py::test_identical_and_duplicated_sets
SPECIAL = {"identical": 5, "copies": 5, "x4": 5, "constant_a": 5, "constant_b": 5}


@functools.lru_cache(maxsize=None)
def special_case(name):
    """(a, b, k, quality_ref64(a, b, k)): B a bitwise copy of A (60 rows); 25 of B's 60 rows copies of rows of A among
    fresh ones; every row of a 30 + 30 pair four times; one constant set of 40 rows against 50 feature-like ones"""
    k, D = SPECIAL[name], 2048
    if name == "identical":
        a = feature_like(5, 60, D)
        b = a.copy()
    elif name == "copies":
        a, b = feature_pair(6, 60, 60, D)
        b = b.copy()
        b[::2][:25] = a[np.random.RandomState(6).permutation(60)[:25]]
    elif name == "x4":
        a, b = (np.repeat(x, 4, axis=0) for x in feature_pair(8, 30, 30, D))
    else:
        a, b = np.full((40, D), 0.37, np.float32), feature_like(9, 50, D)
        if name == "constant_b":
            a, b = b, a
    return a, b, k, quality_ref64(a, b, k)
