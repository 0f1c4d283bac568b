"""Float64 restatement of the six trajectory-metric kernels of csrc/dt_metrics.hip (test infrastructure).

Arrays are numpy, trajectories step-major [n][B][E] float32, as the kernels take them.  The arithmetic is the kernels'
contract, not their summation order:
  * differences are formed in fp32 (as torch forms X_i - Y_i), then widened; squares, products and sums are float64;
  * products x*y, x^2, y^2 use the fp32 inputs widened to float64;
  * row i == 0 of the trajectory sums carries the endpoint terms (include/dt_hip.h, dt_traj_metrics);
  * W1 = mean |sort(u) - sort(v)| over the sampled coordinates, in float64 (NaN in either sample: NaN);
  * the resampled distance uses numpy's linspace (j * (1/(n-1)), last point 1), searchsorted (side left, clipped to
    [1, n-1]) and scipy interp1d's slope * (x - x_lo) + y_lo, all in float64;
  * the sample mean is float32(mean(float64)).
Every sum comes with S, the sum of its terms' magnitudes: the kernels' float64 accumulation (in any order) is within
``sum_bound(S, E)`` of the exact sum, and so is numpy's.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U64 = 2.0 ** -53


def sum_bound(S, count):
    """|got - want| allowed for a float64 sum of ``count`` terms whose magnitudes sum to S."""
    return 4.0 * count * U64 * np.asarray(S, dtype=F64)


def _d32(a, b):
    """fp32 difference, widened (no flush of subnormals; fp32 overflow gives +-inf as on the device)."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32) - np.asarray(b, F32)).astype(F64)


def _w(a):
    return np.asarray(a, F32).astype(F64)


def _sum(t):
    """(sum, sum of magnitudes) over the last axis."""
    with np.errstate(all="ignore"):
        return t.sum(-1), np.abs(t).sum(-1)


def traj_metrics(X, Y):
    """dt_traj_metrics: (sums [B, n_max, 4], S [B, n_max, 4]) for X [nT, B, E], Y [nS, B, E]."""
    nT, B, E = X.shape
    nS = Y.shape[0]
    n = max(nT, nS)
    Xp = np.zeros((n, B, E), F32)
    Yp = np.zeros((n, B, E), F32)
    Xp[:nT], Yp[:nS] = X, Y
    jx = np.array([nT - 1] + list(range(n - 1)))
    jy = np.array([nS - 1] + list(range(n - 1)))
    vx = (np.arange(n) < nT)[:, None, None]
    vy = (np.arange(n) < nS)[:, None, None]
    first = (np.arange(n) == 0)[:, None, None]
    d, dx, dy, de = _d32(Xp, Yp), _d32(Xp, Xp[jx]), _d32(Yp, Yp[jy]), _d32(Xp[jx], Yp[jy])
    with np.errstate(all="ignore"):
        terms = [np.where(vx & vy, d * d, 0.0), np.where(vx, dx * dx, 0.0), np.where(vy, dy * dy, 0.0),
                 np.where(vx & vy, np.where(first, de * de, dx * dy), 0.0)]
    sums, mags = zip(*(_sum(t) for t in terms))                       # each [n, B]
    return np.stack(sums, -1).transpose(1, 0, 2), np.stack(mags, -1).transpose(1, 0, 2)


def pair_stats(X, Y):
    """dt_pair_stats: (out [B, n, 5], S [B, n, 5]) = {sum (x-y)^2, sum |x-y|, sum xy, sum x^2, sum y^2}, X, Y [n, B, E]."""
    d, x, y = _d32(X, Y), _w(X), _w(Y)
    with np.errstate(all="ignore"):
        terms = [d * d, np.abs(d), x * y, x * x, y * y]
    sums, mags = zip(*(_sum(t) for t in terms))
    return np.stack(sums, -1).transpose(1, 0, 2), np.stack(mags, -1).transpose(1, 0, 2)


def w1_sorted(u, v):
    """(W1, S) over the last axis: mean |sort(u) - sort(v)| in float64, S = sum of the |differences|."""
    su, sv = np.sort(_w(u), axis=-1), np.sort(_w(v), axis=-1)
    with np.errstate(all="ignore"):
        t = np.abs(su - sv)
        s = t.sum(-1)
        return s / u.shape[-1], s


def wasserstein(X, Y, index=None, index_row=None):
    """dt_traj_wasserstein: (w1 [B, n], S [B, n]) over the first n = min(len) states.  index [tables, n, cnt] (None: all
    coordinates), index_row [B] (None: table 0)."""
    n = min(X.shape[0], Y.shape[0])
    u, v = X[:n], Y[:n]                                               # [n, B, E]
    if index is not None:
        B = X.shape[1]
        rows = np.zeros(B, np.int64) if index_row is None else np.asarray(index_row, np.int64)
        idx = np.asarray(index, np.int64)[rows][:, :n].transpose(1, 0, 2)      # [n, B, cnt]
        u, v = np.take_along_axis(u, idx, -1), np.take_along_axis(v, idx, -1)
    w, s = w1_sorted(u, v)
    return w.T, s.T


def linspace01(n):
    """numpy.linspace(0, 1, n) as the kernel builds it: j * (1 / (n - 1)), last point exactly 1."""
    if n <= 1:
        return np.zeros(max(n, 0), F64)
    x = np.arange(n, dtype=F64) * (1.0 / (n - 1))
    x[-1] = 1.0
    return x


def resample(L, n_short):
    """Longer trajectory L [n_long, B, E] linearly resampled onto linspace(0, 1, n_short): float64 [n_short, B, E]."""
    n_long = L.shape[0]
    x, x_new = linspace01(n_long), linspace01(n_short)
    hi = np.clip(np.searchsorted(x, x_new, side="left"), 1, n_long - 1)
    lo = hi - 1
    x_lo, x_hi = x[lo][:, None, None], x[hi][:, None, None]
    y_lo, y_hi = _w(L[lo]), _w(L[hi])
    slope = (y_hi - y_lo) / (x_hi - x_lo)
    return slope * (x_new[:, None, None] - x_lo) + y_lo


def resampled_distance(L, S):
    """dt_traj_resampled_distance: float64 [B, n_short] = |L'(t_i) - S_i|_2."""
    d = resample(L, S.shape[0]) - _w(S)
    return np.sqrt((d * d).sum(-1)).T


def sample_mean(traj):
    """dt_traj_sample_mean: float32 [n, E] = mean over the B samples of traj [n, B, E], accumulated in float64."""
    with np.errstate(all="ignore"):
        return _w(traj).mean(axis=1).astype(F32)


NAN, POS_INF, NEG_INF, FINITE = 1, 2, 3, 0


def classes(a):
    """Per element: FINITE, NAN, POS_INF or NEG_INF."""
    a = np.asarray(a)
    c = np.zeros(a.shape, np.int8)
    c[np.isnan(a)] = NAN
    c[np.isposinf(a)] = POS_INF
    c[np.isneginf(a)] = NEG_INF
    return c


def check_sums(got, want, S, count, what):
    """Exact non-finite class, then |got - want| <= sum_bound(S, count) on the finite cells."""
    got, want, S = np.asarray(got, F64), np.asarray(want, F64), np.asarray(S, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    cg, cw = classes(got), classes(want)
    bad = np.argwhere(cg != cw)
    assert bad.size == 0, f"{what}: non-finite class differs at {bad[:5].tolist()}: got {got[tuple(bad[0])]} " \
                          f"want {want[tuple(bad[0])]}"
    ok = cw == FINITE
    err = np.abs(got[ok] - want[ok])
    tol = sum_bound(S[ok], count)
    worst = np.argmax(err - tol) if err.size else None
    assert np.all(err <= tol), f"{what}: |err| {err[worst]:.3e} > bound {tol[worst]:.3e} (want {want[ok][worst]!r})"
