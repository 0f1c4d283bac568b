"""The six trajectory-metric kernels of csrc/dt_metrics.hip against the float64 restatement in tests/metrics_ref64.py.

Each case calls the C ABI directly, twice: once with every output buffer pre-filled with NaN and once with 1e30.  The two
results must be bit-identical (every output cell is written) and must match the restatement:
  * sums and W1: the exact non-finite class (NaN, +inf, -inf or finite) and |got - want| <= 4 E 2^-53 S per cell, S the sum
    of the terms' magnitudes (the cross term <dX, dY> can cancel, so the bound scales with S rather than |want|);
  * resampled distance: 1e-12 relative;  sample mean: 1 fp32 ulp.
Shapes sit where the kernels switch code paths: E around the pair_metrics R = 4 / 8 / 16 boundaries and the +inf padding of
the sorts, E / 4 not a multiple of 256, n up to the 65535 grid limit, B = 65536 (the two-kernel fallback), Wasserstein
tables of 1 .. 4096 coordinates, and a sample mean large enough for its grid-stride loop.  Values: Gaussian trajectories,
integer-quantised ones (ties), X == Y, signed zeros with subnormals, and NaN / +-inf at the first, a middle and the last
coordinate.  The three public functions that reduce through these kernels are also run on entries whose element count is
not a multiple of 4, against oracle/metrics_ref.py.
"""
import math

import numpy as np
import pytest
import torch

import metrics_ref64 as ref64
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd._hip import ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISONS = (float("nan"), 1e30)
DT_E_SHAPE = -2

E_SORT = [4, 8, 12, 764, 768, 772, 1000, 1020, 1024, 1028, 1540, 2044, 2048, 2052, 3072, 4092, 4096]
E_BIG = [12288, 49152]
KINDS = ["gauss", "ties", "same", "zeros"]
# (n, B) per E, rotated so that every n in {1, 2, 3, 51} and every B in {1, 5, 256} meets several E
NB = [(1, 1), (2, 256), (3, 5), (51, 1), (51, 5), (3, 256), (2, 5), (1, 256), (51, 16)]


def _nb(k, E):
    n, B = NB[k % len(NB)]
    while n * B * E > 1 << 21:                                   # keep the float64 restatement small
        B = max(1, B // 4) if B > 1 else B
        n = max(1, n // 2) if B == 1 else n
    return n, B


def _cases(Es):
    out = []
    for k, E in enumerate(Es):
        out.append(pytest.param(E, 3, 5, "gauss", id=f"E{E}-n3-B5-gauss"))
        n, B = _nb(k, E)
        out.append(pytest.param(E, n, B, "gauss", id=f"E{E}-n{n}-B{B}-gauss"))
        for kind in KINDS[1:]:
            out.append(pytest.param(E, 2, 3, kind, id=f"E{E}-n2-B3-{kind}"))
    return out


def _data(kind, nT, nS, B, E, seed):
    """(X [nT, B, E], Y [nS, B, E]) float32."""
    rng = np.random.default_rng(seed)
    n = max(nT, nS)
    if kind == "zeros":
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.17e-38, -1.2e-38], np.float32)
        X = rng.choice(pool, (n, B, E)).astype(np.float32)
        Y = rng.choice(pool, (n, B, E)).astype(np.float32)
    else:
        X = (rng.standard_normal((n, B, E)).cumsum(0) * 0.05).astype(np.float32)
        Y = (X + 0.02 * rng.standard_normal((n, B, E))).astype(np.float32)
        if kind == "ties":
            X, Y = np.round(X * 20).astype(np.float32), np.round(Y * 20).astype(np.float32)
        elif kind == "same":
            Y = X.copy()
    return np.ascontiguousarray(X[:nT]), np.ascontiguousarray(Y[:nS])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _twice(launch, *outs):
    """Run ``launch(*buffers)`` with the output buffers pre-filled with NaN, then with 1e30.  Returns (status, numpy
    outputs); asserts equal status and bit-identical outputs of the two runs."""
    runs = []
    for poison in POISONS:
        bufs = [torch.full(shape, poison, dtype=dt, device=DEV) for shape, dt in outs]
        status = launch(*bufs)
        torch.cuda.synchronize()
        runs.append((status, [b.cpu() for b in bufs]))
    (s0, a), (s1, b) = runs
    assert s0 == s1, (s0, s1)
    if s0 == 0:
        for x, y in zip(a, b):
            ints = torch.int64 if x.dtype == torch.float64 else torch.int32
            diff = (x.view(ints) != y.view(ints)).nonzero()
            assert diff.numel() == 0, f"output cells not written (or read before written): {diff[:5].tolist()}"
    return s0, [x.numpy() for x in b]


# ------------------------------------------------------------------------- raw C ABI launches
def traj_metrics(X, Y):
    nT, B, E = X.shape
    n = max(nT, Y.shape[0])
    Xd, Yd = _dev(X), _dev(Y)
    return _twice(lambda o: _hip.load().dt_traj_metrics(ptr(Xd), ptr(Yd), nT, Y.shape[0], B, E, ptr(o), stream_ptr()),
                  ((B, n, 4), torch.float64))


def pair_metrics(X, Y):
    n, B, E = X.shape
    Xd, Yd = _dev(X), _dev(Y)
    return _twice(lambda s, w: _hip.load().dt_traj_pair_metrics(ptr(Xd), ptr(Yd), n, B, E, ptr(s), ptr(w), stream_ptr()),
                  ((B, n, 4), torch.float64), ((B, n), torch.float64))


def wasserstein(X, Y, index=None, index_row=None):
    n, (_, B, E) = min(X.shape[0], Y.shape[0]), X.shape
    Xd, Yd = _dev(X), _dev(Y)
    idx = None if index is None else _dev(index.astype(np.int32))
    row = None if index_row is None else _dev(np.asarray(index_row, np.int32))
    n_idx = 0 if index is None else index.shape[-1]
    return _twice(lambda o: _hip.load().dt_traj_wasserstein(ptr(Xd), ptr(Yd), n, B, E, ptr(idx), ptr(row), n_idx, ptr(o),
                                                            stream_ptr()),
                  ((B, n), torch.float64))


def resampled_distance(L, S):
    nl, B, E = L.shape
    ns = S.shape[0]
    Ld, Sd = _dev(L), _dev(S)
    return _twice(lambda o: _hip.load().dt_traj_resampled_distance(ptr(Ld), ptr(Sd), nl, ns, B, E, ptr(o), stream_ptr()),
                  ((B, ns), torch.float64))


def pair_stats(X, Y):
    n, B, E = X.shape
    Xd, Yd = _dev(X), _dev(Y)
    return _twice(lambda o: _hip.load().dt_pair_stats(ptr(Xd), ptr(Yd), n, B, E, ptr(o), stream_ptr()),
                  ((B, n, 5), torch.float64))


def sample_mean(T):
    n, B, E = T.shape
    Td = _dev(T)
    return _twice(lambda o: _hip.load().dt_traj_sample_mean(ptr(Td), n, B, E, ptr(o), stream_ptr()), ((n, E), torch.float32))


def _ok(res):
    status, outs = res
    assert status == 0, _hip.load().dt_status_string(status)
    return outs if len(outs) > 1 else outs[0]


def _check_w1(got, X, Y, what, index=None, index_row=None):
    want, S = ref64.wasserstein(X, Y, index, index_row)
    cnt = X.shape[-1] if index is None else index.shape[-1]
    # the restatement returns the mean: its bound is the sum's bound over cnt
    ref64.check_sums(got, want, S / cnt, cnt, what)


# ------------------------------------------------------------------------- finite values at the path boundaries
@pytest.mark.parametrize("E,n,B,kind", _cases(E_SORT + E_BIG))
def test_traj_metrics_vs_float64(E, n, B, kind):
    X, Y = _data(kind, n, n, B, E, seed=E * 7 + n)
    got = _ok(traj_metrics(X, Y))
    want, S = ref64.traj_metrics(X, Y)
    ref64.check_sums(got, want, S, E, "traj_metrics")
    if kind == "same":
        assert not got[..., 0].any()


@pytest.mark.parametrize("nT,nS", [(21, 6), (6, 21), (1, 5), (5, 1), (51, 11)])
@pytest.mark.parametrize("E", [12, 772])
def test_traj_metrics_unequal_lengths_vs_float64(nT, nS, E):
    """Rows beyond a trajectory's own length carry 0 for every term that needs one of its states."""
    X, Y = _data("gauss", nT, nS, 3, E, seed=nT * 100 + nS)
    got = _ok(traj_metrics(X, Y))
    want, S = ref64.traj_metrics(X, Y)
    ref64.check_sums(got, want, S, E, "traj_metrics")
    short = min(nT, nS)
    assert not got[:, short:, 0].any() and not got[:, short:, 3].any()
    assert not got[:, nT:, 1].any() and not got[:, nS:, 2].any()


@pytest.mark.parametrize("E,n,B,kind", _cases(E_SORT))
def test_pair_metrics_vs_float64(E, n, B, kind):
    """The one-pass kernel (sums + register / cross-lane / LDS bitonic sort) for R = 4, 8, 16 coordinates per thread."""
    X, Y = _data(kind, n, n, B, E, seed=E * 11 + n)
    sums, w1 = _ok(pair_metrics(X, Y))
    want, S = ref64.traj_metrics(X, Y)
    ref64.check_sums(sums, want, S, E, "pair_metrics sums")
    _check_w1(w1, X, Y, "pair_metrics W1")
    if kind == "same":
        assert not w1.any() and not sums[..., 0].any()


@pytest.mark.parametrize("E,n,B,kind", _cases(E_SORT))
def test_wasserstein_all_coordinates_vs_float64(E, n, B, kind):
    """dt_traj_wasserstein with index = NULL: the LDS bitonic sort padded to 1024 / 2048 / 4096 with +inf."""
    X, Y = _data(kind, n, n, B, E, seed=E * 13 + n)
    w1 = _ok(wasserstein(X, Y))
    _check_w1(w1, X, Y, "wasserstein W1")
    if kind == "same":
        assert not w1.any()


def _tables(E, n, cnt, seed, tables=3):
    rng = np.random.default_rng(seed)
    idx = np.stack([np.stack([rng.choice(E, cnt, replace=False) for _ in range(n)]) for _ in range(tables)])
    idx[1, n - 1, cnt // 2] = E - 1                               # the last coordinate is sampled
    return idx.astype(np.int32)


@pytest.mark.parametrize("cnt", [1, 2, 3, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096])
@pytest.mark.parametrize("kind", ["gauss", "ties"])
def test_wasserstein_tables_vs_float64(cnt, kind):
    """Sub-sampled tables: pairs mapped to distinct and repeated tables, an index equal to E - 1."""
    n, B, E = 3, 5, 4099
    X, Y = _data(kind, n, n, B, E, seed=cnt)
    index, rows = _tables(E, n, cnt, seed=cnt + 1), np.array([2, 0, 2, 1, 0], np.int32)
    w1 = _ok(wasserstein(X, Y, index, rows))
    _check_w1(w1, X, Y, "wasserstein W1 (tables)", index, rows)
    # table 0 for every pair when index_row is NULL
    w1_0 = _ok(wasserstein(X, Y, index))
    _check_w1(w1_0, X, Y, "wasserstein W1 (table 0)", index, None)


@pytest.mark.parametrize("E,n,B,kind", _cases(E_SORT + E_BIG))
def test_pair_stats_vs_float64(E, n, B, kind):
    X, Y = _data(kind, n, n, B, E, seed=E * 17 + n)
    got = _ok(pair_stats(X, Y))
    want, S = ref64.pair_stats(X, Y)
    ref64.check_sums(got, want, S, E, "pair_stats")


@pytest.mark.parametrize("n_long,n_short", [(2, 1), (2, 2), (3, 2), (21, 6), (51, 11), (51, 50), (101, 51), (1001, 3)])
@pytest.mark.parametrize("E", [1, 3, 770, 1028])
def test_resampled_distance_vs_float64(n_long, n_short, E):
    B = 3 if n_long * E < 200000 else 1
    L, S = _data("gauss", n_long, n_short, B, E, seed=n_long * 1000 + n_short)
    got = _ok(resampled_distance(L, S))
    want = ref64.resampled_distance(L, S)
    assert np.all(np.abs(got - want) <= 1e-12 * want), np.abs(got - want).max()


@pytest.mark.parametrize("E", E_BIG)
def test_resampled_distance_large_entries_vs_float64(E):
    L, S = _data("gauss", 21, 6, 2, E, seed=E)
    got = _ok(resampled_distance(L, S))
    want = ref64.resampled_distance(L, S)
    assert np.all(np.abs(got - want) <= 1e-12 * want), np.abs(got - want).max()


def _check_mean(got, want):
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(ref64.classes(got), ref64.classes(want))
    ok = np.isfinite(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    ulp = np.spacing(np.abs(want[ok]))
    assert np.all(err <= ulp), (err / ulp).max()


@pytest.mark.parametrize("n,B,E", [(1, 1, 1), (3, 1000, 7), (51, 256, 768), (51, 16, 12288)])
@pytest.mark.parametrize("kind", ["gauss", "zeros"])
def test_sample_mean_vs_float64(n, B, E, kind):
    """(51, 16, 12288) is past 2048 blocks of 256 outputs: the grid-stride loop runs."""
    T, _ = _data(kind, n, 1, B, E, seed=n * B + E)
    _check_mean(_ok(sample_mean(T)), ref64.sample_mean(T))


def test_sample_mean_keeps_non_finite_samples_in_their_cell():
    T, _ = _data("gauss", 3, 1, 4, 9, seed=1)
    T[1, 3, 8], T[2, 0, 0], T[2, 1, 4], T[2, 2, 4] = np.nan, np.inf, np.inf, -np.inf
    _check_mean(_ok(sample_mean(T)), ref64.sample_mean(T))


# ------------------------------------------------------------------------- grid limits
@pytest.mark.parametrize("kernel", ["traj_metrics", "pair_metrics", "wasserstein", "pair_stats", "resampled_distance"])
def test_step_count_limit(kernel):
    """n = 65535 steps (the grid's y limit) are computed; 65536 are rejected with DT_E_SHAPE and nothing written."""
    E, B = 4, 1
    for n, ok in ((65535, True), (65536, False)):
        X, Y = _data("gauss", n + (kernel == "resampled_distance"), n, B, E, seed=n)
        status, outs = {"traj_metrics": traj_metrics, "pair_metrics": pair_metrics, "wasserstein": wasserstein,
                        "pair_stats": pair_stats, "resampled_distance": resampled_distance}[kernel](X, Y)
        if not ok:
            assert status == DT_E_SHAPE and all(np.all(o == 1e30) for o in outs), status
            continue
        assert status == 0, status
        if kernel == "resampled_distance":
            want = ref64.resampled_distance(X, Y)
            assert np.all(np.abs(outs[0] - want) <= 1e-12 * want)
            continue
        if kernel in ("traj_metrics", "pair_metrics"):
            want, S = ref64.traj_metrics(X, Y)
            ref64.check_sums(outs[0], want, S, E, kernel)
        if kernel == "pair_stats":
            want, S = ref64.pair_stats(X, Y)
            ref64.check_sums(outs[0], want, S, E, kernel)
        if kernel in ("pair_metrics", "wasserstein"):
            _check_w1(outs[-1], X, Y, kernel)


def test_pair_metrics_large_batch_takes_the_two_kernel_path():
    """B = 65536 pairs exceed the one-pass kernel's grid (rejected cleanly); device_pair_metrics then takes
    dt_traj_metrics + dt_traj_wasserstein and gives the float64 values."""
    n, B, E = 2, 65536, 8
    X, Y = _data("gauss", n, n, B, E, seed=5)
    status, _ = pair_metrics(X, Y)
    assert status == DT_E_SHAPE
    sums, w1 = engine.device_pair_metrics(_dev(X), _dev(Y))
    want, S = ref64.traj_metrics(X, Y)
    ref64.check_sums(sums.cpu().numpy(), want, S, E, "fallback sums")
    _check_w1(w1.cpu().numpy(), X, Y, "fallback W1")


# ------------------------------------------------------------------------- non-finite values
VALUES = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}
POSITIONS = ("first", "mid", "last")
PLACES = ("X", "Y", "both", "prev")


def _poisoned(E, val, pos, place, n=3, B=2):
    """Trajectories with one non-finite coordinate: in X_1, Y_1, both, or X_0 only (the previous state of step 1)."""
    X, Y = _data("gauss", n, n, B, E, seed=E)
    e = {"first": 0, "mid": E // 2 + 1, "last": E - 1}[pos] if isinstance(pos, str) else pos
    v = VALUES[val]
    if place in ("X", "both"):
        X[1, 1, e] = v
    if place in ("Y", "both"):
        Y[1, 1, e] = v
    if place == "prev":
        X[0, 1, e] = v
    return X, Y


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("val", list(VALUES))
@pytest.mark.parametrize("E", [768, 1540])
@pytest.mark.parametrize("path", ["pair_metrics", "two_kernel"])
def test_non_finite_cells(path, E, val, pos, place):
    """The exact NaN / +inf / -inf class of every cell, through the one-pass kernel and through traj_metrics + wasserstein;
    the last coordinate is the one a NaN-blind sort loses into the +inf padding."""
    X, Y = _poisoned(E, val, pos, place)
    if path == "pair_metrics":
        sums, w1 = _ok(pair_metrics(X, Y))
    else:
        sums, w1 = _ok(traj_metrics(X, Y)), _ok(wasserstein(X, Y))
    want, S = ref64.traj_metrics(X, Y)
    ref64.check_sums(sums, want, S, E, f"{path} sums")
    _check_w1(w1, X, Y, f"{path} W1")


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("val", list(VALUES))
def test_wasserstein_tables_non_finite_cells(val, pos, place):
    """cnt = 1000 coordinates in N = 1024 slots through a table: the non-finite value at the first, a middle and the last
    SAMPLED coordinate."""
    n, B, E, cnt = 3, 2, 1540, 1000
    index = _tables(E, n, cnt, seed=9, tables=2)
    rows = np.array([1, 0], np.int32)
    k = {"first": 0, "mid": cnt // 2 + 1, "last": cnt - 1}[pos]
    X, Y = _poisoned(E, val, int(index[rows[1], 1 if place != "prev" else 0, k]), place, n, B)
    w1 = _ok(wasserstein(X, Y, index, rows))
    _check_w1(w1, X, Y, "wasserstein W1 (tables)", index, rows)


@pytest.mark.parametrize("E", [768, 1540])
def test_non_finite_subnormal_and_signed_zero_mix(E):
    """Signed zeros, subnormals and one NaN / +inf / -inf per pair in one tensor: classes and values per cell."""
    X, Y = _data("zeros", 4, 4, 3, E, seed=E)
    X[2, 0, E - 1], Y[3, 1, 0], X[1, 2, E // 3], Y[1, 2, E // 3] = np.nan, np.inf, -np.inf, -np.inf
    for path in ("pair_metrics", "two_kernel"):
        sums, w1 = _ok(pair_metrics(X, Y)) if path == "pair_metrics" else (_ok(traj_metrics(X, Y)), _ok(wasserstein(X, Y)))
        want, S = ref64.traj_metrics(X, Y)
        ref64.check_sums(sums, want, S, E, f"{path} sums")
        _check_w1(w1, X, Y, f"{path} W1")
    got = _ok(pair_stats(X, Y))
    want, S = ref64.pair_stats(X, Y)
    ref64.check_sums(got, want, S, E, "pair_stats")


# ------------------------------------------------------------------------- public functions on E % 4 != 0 entries
def _close(got, want, what, rel=2e-5):
    if isinstance(want, dict):
        assert set(got) >= set(want), what
        for k in want:
            _close(got[k], want[k], f"{what}.{k}", rel)
        return
    if isinstance(want, (list, tuple)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            _close(g, w, f"{what}[{i}]", rel)
        return
    if want is None or isinstance(want, str):
        assert got == want, what
        return
    g, w = float(got), float(want)
    if math.isnan(w) or math.isinf(w):
        assert (math.isnan(g) and math.isnan(w)) or g == w, (what, g, w)
        return
    assert abs(g - w) <= rel * abs(w) + 1e-7, (what, g, w)


ODD_SHAPES = [(1, 1, 5, 5), (1, 3, 7, 7)]


def _odd_traj(shape, n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(shape, generator=g) * scale).cumsum(-1) * 0.1 for _ in range(n)]


@pytest.mark.parametrize("nT,nS", [(6, 6), (9, 5)])
@pytest.mark.parametrize("shape", ODD_SHAPES, ids=["1x1x5x5", "1x3x7x7"])
def test_compute_trajectory_metrics_on_odd_entries(shape, nT, nS):
    from distillation_trajectories_amd.analysis.metrics.trajectory_metrics import compute_trajectory_metrics
    from oracle import metrics_ref
    X = _odd_traj(shape, nT, 1)
    g = torch.Generator().manual_seed(2)
    Y = [x + 1e-3 * torch.randn(shape, generator=g) for x in _odd_traj(shape, nS, 1)]
    np.random.seed(0)
    got = compute_trajectory_metrics(X, Y)
    np.random.seed(0)
    want = metrics_ref.compute_trajectory_metrics(X, Y)
    _close(got, want, "compute_trajectory_metrics")


@pytest.mark.parametrize("shape", ODD_SHAPES, ids=["1x1x5x5", "1x3x7x7"])
def test_compute_trajectory_divergence_on_odd_entries(shape):
    from distillation_trajectories_amd.evaluation.metrics import compute_trajectory_divergence
    from oracle import metrics_ref
    a = [(x, t) for t, x in enumerate(_odd_traj(shape, 7, 3))]
    b = [(x, t) for t, x in enumerate(_odd_traj(shape, 5, 4))]
    _close(compute_trajectory_divergence(a, b), metrics_ref.trajectory_divergence(a, b), "compute_trajectory_divergence")


@pytest.mark.parametrize("shape", ODD_SHAPES, ids=["1x1x5x5", "1x3x7x7"])
def test_analyze_time_dependent_distances_on_odd_entries(shape):
    from distillation_trajectories_amd.analysis.metrics.time_dependent import analyze_time_dependent_distances
    from oracle import metrics_ref
    teacher = [_odd_traj(shape, 6, 10 + k) for k in range(3)]
    student = [_odd_traj(shape, 4, 20 + k) for k in range(2)] + [_odd_traj(shape, 6, 30)]
    got = analyze_time_dependent_distances(teacher, student, None)
    want = metrics_ref.time_dependent_distances(teacher, student)
    _close({k: got[k] for k in want}, want, "analyze_time_dependent_distances")
