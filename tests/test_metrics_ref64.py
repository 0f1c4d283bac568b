"""CPU checks of the float64 restatement in tests/metrics_ref64.py, the reference of tests/test_hip_metrics.py.

W1 is checked against scipy.stats.wasserstein_distance (including its NaN / +-inf classes), the vectorised resample
against per-coordinate scipy interp1d, and the sums against plain per-cell loops."""
import math

import numpy as np
import pytest
from scipy.interpolate import interp1d
from scipy.stats import wasserstein_distance

import metrics_ref64 as ref64


@pytest.mark.parametrize("E", [1, 2, 3, 7, 768, 1000])
def test_w1_matches_scipy(E):
    rng = np.random.default_rng(E)
    for u, v in ((rng.standard_normal(E), rng.standard_normal(E)),
                 (np.round(rng.standard_normal(E) * 2), np.round(rng.standard_normal(E) * 2)),   # many ties
                 (rng.standard_normal(E) * 1e-40, rng.standard_normal(E) * 1e-40)):              # fp32 subnormals
        u, v = u.astype(np.float32), v.astype(np.float32)
        w, _ = ref64.w1_sorted(u, v)
        want = wasserstein_distance(u.astype(np.float64), v.astype(np.float64))
        assert abs(w - want) <= 1e-12 * max(abs(want), 1e-300) + 1e-300, (w, want)
        assert ref64.w1_sorted(u, u)[0] == 0.0


@pytest.mark.parametrize("pos", [0, 100, 767])
@pytest.mark.parametrize("case,cls", [("nan_u", ref64.NAN), ("nan_v", ref64.NAN), ("nan_both", ref64.NAN),
                                      ("pinf_u", ref64.POS_INF), ("ninf_v", ref64.POS_INF), ("pinf_both", ref64.NAN),
                                      ("ninf_both", ref64.NAN), ("pinf_u_ninf_v", ref64.POS_INF)])
def test_w1_non_finite_classes_match_scipy(case, cls, pos):
    """One-sided +-inf gives +inf, the same infinity in both samples NaN, a NaN anywhere NaN: the class scipy gives."""
    rng = np.random.default_rng(pos)
    u, v = rng.standard_normal(768).astype(np.float32), rng.standard_normal(768).astype(np.float32)
    val = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}
    parts = case.split("_")
    if parts[-1] == "both":
        u[pos] = v[pos] = val[parts[0]]
    elif len(parts) == 4:
        u[pos], v[pos] = val[parts[0]], val[parts[2]]
    else:
        (u if parts[1] == "u" else v)[pos] = val[parts[0]]
    w, _ = ref64.w1_sorted(u, v)
    with np.errstate(all="ignore"):
        want = wasserstein_distance(u.astype(np.float64), v.astype(np.float64))
    assert ref64.classes(w) == ref64.classes(want) == cls, (w, want)


@pytest.mark.parametrize("n_long,n_short", [(2, 1), (2, 2), (3, 2), (21, 6), (51, 11), (51, 50), (101, 51), (1001, 3)])
@pytest.mark.parametrize("E", [1, 3, 5])
def test_resample_matches_scipy_interp1d(n_long, n_short, E):
    rng = np.random.default_rng(n_long * 100 + n_short)
    B = 2
    L = rng.standard_normal((n_long, B, E)).astype(np.float32)
    S = rng.standard_normal((n_short, B, E)).astype(np.float32)
    got = ref64.resample(L, n_short)
    x, x_new = np.linspace(0, 1, n_long), np.linspace(0, 1, n_short)
    assert np.array_equal(ref64.linspace01(n_long), x) and np.array_equal(ref64.linspace01(n_short), x_new)
    for b in range(B):
        for e in range(E):
            # a 2-D y keeps interp1d on its own slope * (x - x_lo) + y_lo (a 1-D float64 y is handed to numpy.interp)
            f = interp1d(x, L[:, b, e:e + 1].astype(np.float64), kind="linear", axis=0)
            assert f._call.__name__ == "_call_linear"
            assert np.array_equal(got[:, b, e], f(x_new)[:, 0]), (b, e)
    d = ref64.resampled_distance(L, S)
    for b in range(B):
        for i in range(n_short):
            assert d[b, i] == math.sqrt(float(((got[i, b] - S[i, b].astype(np.float64)) ** 2).sum()))


@pytest.mark.parametrize("nT,nS", [(3, 3), (21, 6), (6, 21), (1, 5), (5, 1)])
def test_traj_metrics_restatement_matches_loops(nT, nS):
    rng = np.random.default_rng(nT * 10 + nS)
    B, E = 2, 12
    X = rng.standard_normal((nT, B, E)).astype(np.float32)
    Y = rng.standard_normal((nS, B, E)).astype(np.float32)
    got, S = ref64.traj_metrics(X, Y)
    f = np.float64
    for b in range(B):
        for i in range(max(nT, nS)):
            want = [0.0] * 4
            if i < nT and i < nS:
                want[0] = sum(f(x - y) ** 2 for x, y in zip(X[i, b], Y[i, b]))
            px = X[i - 1 if i else nT - 1, b] if i < nT else None
            py = Y[i - 1 if i else nS - 1, b] if i < nS else None
            if i < nT:
                want[1] = sum(f(a - p) ** 2 for a, p in zip(X[i, b], px))
            if i < nS:
                want[2] = sum(f(a - p) ** 2 for a, p in zip(Y[i, b], py))
            if i < nT and i < nS:
                want[3] = (sum(f(a - p) * f(c - q) for a, p, c, q in zip(X[i, b], px, Y[i, b], py)) if i else
                           sum(f(p - q) ** 2 for p, q in zip(px, py)))
            ref64.check_sums(got[b, i], np.array(want), S[b, i], E, f"b{b} i{i}")


def test_pair_stats_and_sample_mean_restatement():
    rng = np.random.default_rng(7)
    X = rng.standard_normal((3, 4, 9)).astype(np.float32)
    Y = rng.standard_normal((3, 4, 9)).astype(np.float32)
    got, S = ref64.pair_stats(X, Y)
    f = np.float64
    for b in range(4):
        for i in range(3):
            x, y = X[i, b], Y[i, b]
            want = [sum(f(d) ** 2 for d in x - y), sum(abs(f(d)) for d in x - y), sum(f(a) * f(c) for a, c in zip(x, y)),
                    sum(f(a) ** 2 for a in x), sum(f(c) ** 2 for c in y)]
            ref64.check_sums(got[b, i], np.array(want), S[b, i], 9, f"b{b} i{i}")
    m = ref64.sample_mean(X)
    assert m.dtype == np.float32 and np.array_equal(m, np.float32(X.astype(f).sum(1) / 4))


def test_sums_keep_fp32_differences_and_subnormals():
    """Differences are fp32 (rounded) and subnormal differences are not flushed."""
    X = np.array([[[1.0 + 2.0 ** -23, 1e-45, 3e-39, 0.0]]], np.float32)
    Y = np.array([[[2.0 ** -30, -1e-45, -0.0, -0.0]]], np.float32)
    out, _ = ref64.pair_stats(X, Y)
    d = (X - Y).astype(np.float64)[0, 0]
    assert d[1] > 0 and d[2] > 0 and d[3] == 0
    assert out[0, 0, 1] == np.abs(d).sum() and out[0, 0, 0] == (d * d).sum()
    assert d[0] == np.float64(np.float32(1.0 + 2.0 ** -23) - np.float32(2.0 ** -30)) != 1.0 + 2.0 ** -23 - 2.0 ** -30
