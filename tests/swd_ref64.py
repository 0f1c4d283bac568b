"""The yardstick for the sliced Wasserstein distance (include/dt_hip_swd.h), in plain numpy.

Projections proj[l][i] = sum_e theta[l][e] x[i][e] with every product and sum in ``np.longdouble`` (x87 extended: unit
roundoff 2^-64, 2048 times below fp64's), ``np.sort`` per direction, then the exact W_p^p between the two empirical
quantile functions, as the header defines it: with "big" the larger set (A on a tie, sizes nB >= nS), element i of big
overlaps elements j = floor(i nS / nB) .. ceil((i+1) nS / nB) - 1 of small with the integer weight
w_ij = min((i+1) nS, (j+1) nB) - max(i nS, j nB), and  W_p^p = sum_ij w_ij |big_i - small_j|^p / (nB nS).

``forward_bound`` is the a-priori tolerance for a device output, derived from the number formats, never from what the
device returns.  With u = 2^-53:

  * a projection computed in fp64 as one chain of E fused multiply-adds of exact products is within
    delta_i = E u sum_e |theta_e x_ie| of the true one; delta_a is the largest delta_i of set A, delta = delta_a + delta_b;
  * sorting is non-expansive in the max norm: the k-th smallest of the computed projections is within delta_a of the k-th
    smallest of the true ones;
  * so every difference big_i - small_j moves by at most delta, and with D the largest true |big_i - small_j| over the
    overlapping pairs its p-th power moves by at most p (D + delta)^(p-1) delta; the weights are exact, non-negative
    and add up to nB nS, so the weighted mean moves by no more;
  * the subtraction, the square, the fused multiply-add, the at most ceil(nS / nB) + 1 terms of a chain, the
    ceil(log2 nB) levels of the tree and the division each lose at most u of a non-negative partial sum: fewer than
    n_a + n_b + 8 roundings in all, hence
        |w - w_ref| <= p (D + delta)^(p-1) delta + (n_a + n_b + 8) u w_ref;
  * mean_w adds the totals of the L directions in a tree of ceil(log2 L) levels and divides once:
        |mean_w - mean_ref| <= mean_l bound_l + (ceil(log2 L) + 2) u mean_ref;
  * max_w is the largest w: |max_w - max_ref| <= max_l bound_l.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53                     # unit roundoff of fp64


def project(theta, x):
    """[.., L, n] extended-precision projections of the rows x [.., n, E] onto theta [L, E]"""
    return np.einsum("le,...ne->...ln", np.asarray(theta).astype(LD), np.asarray(x).astype(LD))


def overlaps(n_big, n_small):
    """(i, j, w): the overlapping pairs of the two quantile functions and their integer weights, i ascending then j"""
    cuts = np.unique(np.concatenate([np.arange(n_big + 1) * n_small, np.arange(n_small + 1) * n_big]))
    lo, hi = cuts[:-1], cuts[1:]
    return lo // n_small, lo // n_big, hi - lo


def quantile_distance(a_sorted, b_sorted, p):
    """W_p^p between two sorted samples (last axis), in the dtype of the inputs"""
    n_a, n_b = a_sorted.shape[-1], b_sorted.shape[-1]
    big, small = (a_sorted, b_sorted) if n_a >= n_b else (b_sorted, a_sorted)
    i, j, w = overlaps(big.shape[-1], small.shape[-1])
    d = np.abs(big[..., i] - small[..., j])
    return (w.astype(d.dtype) * d ** p).sum(axis=-1) / d.dtype.type(n_a * n_b)


def status(a, b, theta):
    """[P] int: 1 where a problem's rows (of either set) or theta hold a NaN or Inf.  a, b [P, n, E] (or [n, E]: shared)"""
    bad = ~np.isfinite(np.asarray(theta)).all()
    flags = [~np.isfinite(np.asarray(x).reshape((-1,) + np.asarray(x).shape[-2:])).all(axis=(1, 2)) for x in (a, b)]
    return ((flags[0] | flags[1]) | bad).astype(np.int32)


def delta(theta, x):
    """[.., L]: the largest delta_i = E u sum_e |theta_e x_ie| over the rows of x.  The sum of magnitudes is formed in
    float64 and raised by 1e-9 of itself, far above its own rounding (E 2^-53), so that it stays an upper bound."""
    mag = np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(np.asarray(theta, dtype=np.float64)).T       # [.., n, L]
    return (np.asarray(theta).shape[-1] * U * (1 + 1e-9)) * mag.max(axis=-2).astype(LD)


class Case:
    """Sets a [.., n_a, E] and b [.., n_b, E] against theta [L, E]: the sorted extended-precision projections are made
    once; ``swd`` and ``forward_bound`` then serve any p, and any leading ``L`` directions (a direction's result does not
    depend on the others)."""

    def __init__(self, a, b, theta):
        self.sa, self.sb = np.sort(project(theta, a), axis=-1), np.sort(project(theta, b), axis=-1)
        self.delta = delta(theta, a) + delta(theta, b)
        self.n_a, self.n_b = self.sa.shape[-1], self.sb.shape[-1]
        big, small = (self.sa, self.sb) if self.n_a >= self.n_b else (self.sb, self.sa)
        i, j, _ = overlaps(big.shape[-1], small.shape[-1])
        self.D = np.abs(big[..., i] - small[..., j]).max(axis=-1)
        self.w = {}

    def _w(self, p):
        if p not in self.w:
            self.w[p] = quantile_distance(self.sa, self.sb, p)
        return self.w[p]

    def swd(self, p, L=None):
        """{w [.., L], mean_w [..], max_w [..], argmax [..]} in extended precision"""
        w = self._w(p)[..., :L]
        return {"w": w, "mean_w": w.mean(axis=-1), "max_w": w.max(axis=-1), "argmax": w.argmax(axis=-1)}

    def forward_bound(self, p, L=None):
        """{w [.., L], mean_w [..], max_w [..]}: the bounds of the module docstring"""
        ref, D, dl = self._w(p)[..., :L], self.D[..., :L], self.delta[..., :L]
        w = p * (D + dl) ** (p - 1) * dl + (self.n_a + self.n_b + 8) * U * ref
        n = ref.shape[-1]
        levels = int(np.ceil(np.log2(n))) if n > 1 else 0
        return {"w": w, "mean_w": w.mean(axis=-1) + (levels + 2) * U * ref.mean(axis=-1), "max_w": w.max(axis=-1)}


def swd(a, b, theta, p):
    return Case(a, b, theta).swd(p)


def forward_bound(a, b, theta, p):
    return Case(a, b, theta).forward_bound(p)


# ------------------------------------------------------------------------------------------------ test inputs
KINDS = ("gauss", "offset", "near", "ties")


def sets(seed, P, n_a, n_b, E, kind):
    """(a [P, n_a, E], b [P, n_b, E]) float32"""
    rng = np.random.RandomState(seed)
    a, b = rng.standard_normal((P, n_a, E)), 0.5 + 1.25 * rng.standard_normal((P, n_b, E))
    if kind == "offset":
        a, b = a + 100.0, b + 100.0
    elif kind == "near":
        b = a[:, np.arange(n_b) % n_a] + 1e-6 * rng.standard_normal((P, n_b, E))
    elif kind == "ties":
        a, b = rng.randint(-1, 2, (P, n_a, E)).astype(np.float64), rng.randint(-1, 2, (P, n_b, E)).astype(np.float64)
    elif kind != "gauss":
        raise ValueError(kind)
    return a.astype(np.float32), b.astype(np.float32)


def unit_directions(seed, L, E):
    """[L, E] float32 rows of unit norm (to float32 rounding) from numpy's generator: the tests' own, not engine.swd_directions"""
    d = np.random.RandomState(seed).standard_normal((L, E))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
