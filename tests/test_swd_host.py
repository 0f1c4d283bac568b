"""Sliced Wasserstein distance without a GPU: the yardstick swd_ref64 against scipy and against closed forms, the
directions, the derived Python quantities, the exported surface of include/dt_hip_swd.h, the size queries, the sanitizer
driver, and argument checks that fail before any device call."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy.stats import wasserstein_distance

import swd_ref64 as ref
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.analysis import metrics
from distillation_trajectories_amd.analysis.metrics import sliced_wasserstein as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dt_hip_swd.h")
SIZES = [(5, 5), (7, 3), (3, 7), (6, 4), (64, 48), (1, 9)]


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("n_a,n_b", SIZES)
def test_yardstick_equals_scipy_for_p_1(n_a, n_b):
    rng = np.random.RandomState(n_a * 100 + n_b)
    a, b = rng.standard_normal(n_a), 0.5 + 2.0 * rng.standard_normal(n_b)
    got = float(ref.quantile_distance(np.sort(a).astype(ref.LD), np.sort(b).astype(ref.LD), 1))
    want = wasserstein_distance(a, b)
    assert abs(got - want) <= 1e-14 * want
    swapped = float(ref.quantile_distance(np.sort(b).astype(ref.LD), np.sort(a).astype(ref.LD), 1))
    assert abs(swapped - got) <= 1e-17 * got


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_yardstick_at_equal_sizes_for_p_2(n):
    rng = np.random.RandomState(n)
    a, b = np.sort(rng.standard_normal(n)).astype(ref.LD), np.sort(3.0 * rng.standard_normal(n)).astype(ref.LD)
    want = ((a - b) ** 2).mean()
    assert abs(ref.quantile_distance(a, b, 2) - want) <= 1e-17 * want
    i, j, w = ref.overlaps(n, n)
    assert i.tolist() == j.tolist() == list(range(n)) and (w == n).all()


@pytest.mark.parametrize("n_a,n_b", [(7, 3), (6, 4), (64, 48)])
@pytest.mark.parametrize("p", [1, 2])
def test_yardstick_at_unequal_sizes_equals_replicated_samples(n_a, n_b, p):
    """n_b/g copies of every a and n_a/g copies of every b are two samples of lcm(n_a, n_b) with the same distributions"""
    rng = np.random.RandomState(n_a + n_b + p)
    a, b = np.sort(rng.standard_normal(n_a)).astype(ref.LD), np.sort(1.0 + rng.standard_normal(n_b)).astype(ref.LD)
    g = np.gcd(n_a, n_b)
    ra, rb = np.repeat(a, n_b // g), np.repeat(b, n_a // g)
    want = (np.abs(ra - rb) ** p).mean()
    assert abs(ref.quantile_distance(a, b, p) - want) <= 1e-17 * want
    i, j, w = ref.overlaps(max(n_a, n_b), min(n_a, n_b))
    nB, nS = max(n_a, n_b), min(n_a, n_b)
    assert w.sum() == n_a * n_b and (w > 0).all()
    assert (j >= i * nS // nB).all() and (j <= -((-(i + 1) * nS) // nB) - 1).all()            # the header's range of j
    assert (w == np.minimum((i + 1) * nS, (j + 1) * nB) - np.maximum(i * nS, j * nB)).all()   # and its weight


def test_yardstick_swd_and_bound_shapes():
    a, b = ref.sets(1, 3, 7, 3, 5, "gauss")
    theta = ref.unit_directions(2, 4, 5)
    r, bound = ref.swd(a, b, theta, 2), ref.forward_bound(a, b, theta, 2)
    assert r["w"].shape == bound["w"].shape == (3, 4) and r["mean_w"].shape == bound["mean_w"].shape == (3,)
    assert (r["max_w"] == r["w"].max(axis=1)).all() and (r["argmax"] == r["w"].argmax(axis=1)).all()
    assert (bound["w"] > 0).all() and (bound["w"] < 1e-12 * r["w"]).all()             # a tolerance, not a loophole
    plain = ref.quantile_distance(np.sort(ref.project(theta, a).astype(np.float64), axis=-1),
                                  np.sort(ref.project(theta, b).astype(np.float64), axis=-1), 2)
    assert (np.abs(plain - r["w"]) <= bound["w"]).all()                                # plain float64 meets it
    assert ref.status(a, b, theta).tolist() == [0, 0, 0]
    a[1, 2, 3] = np.nan
    assert ref.status(a, b, theta).tolist() == [0, 1, 0]
    theta[0, 0] = np.inf
    assert ref.status(a, b, theta).tolist() == [1, 1, 1]
    for kind in ref.KINDS:
        x, y = ref.sets(3, 2, 4, 6, 3, kind)
        assert x.shape == (2, 4, 3) and y.shape == (2, 6, 3) and x.dtype == y.dtype == np.float32


def test_integer_data_is_exact_in_the_yardstick():
    rng = np.random.RandomState(5)
    a, b = np.sort(rng.randint(-9, 10, 6)), np.sort(rng.randint(-9, 10, 4))
    i, j, w = ref.overlaps(6, 4)
    exact = Fraction(int((w * (a[i] - b[j]) ** 2).sum()), 24)
    assert float(ref.quantile_distance(a.astype(ref.LD), b.astype(ref.LD), 2)) == float(exact)


# ------------------------------------------------------------------------------------------------ directions
def test_directions_are_unit_deterministic_and_private():
    torch.manual_seed(123)
    before = torch.get_rng_state().clone()
    d = engine.swd_directions(48, 16, seed=3)
    assert torch.equal(torch.get_rng_state(), before)                 # the global generator is neither read nor advanced
    assert d.dtype == torch.float32 and tuple(d.shape) == (16, 48) and d.device.type == "cpu"
    norms = d.double().norm(dim=1)
    assert (norms - 1).abs().max() <= 48 ** 0.5 * 2.0 ** -24          # every element rounded to float32 once
    assert engine.swd_directions(48, 16, seed=3) is d                 # kept per (E, L, seed)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(3)
    raw = torch.randn(16, 48, dtype=torch.float64, generator=gen)
    assert torch.equal(d, (raw / raw.norm(dim=1, keepdim=True)).float())
    assert not torch.equal(engine.swd_directions(48, 16, seed=4), d)
    assert engine.swd_directions(1, 2).abs().tolist() == [[1.0], [1.0]]
    for bad in ((0, 4), (4, 0), (4, 4097), ((1 << 20) + 1, 1), (4.0, 4), (True, 4), (4, 4, -1), (4, 4, 1.5)):
        with pytest.raises(ValueError):
            engine.swd_directions(*bad)


# ------------------------------------------------------------------------------------------------ derived quantities
def test_derived_distances():
    swd, mx = sw.derived_distances(np.array([4.0, 0.0, np.nan]), np.array([9.0, 0.0, np.nan]), 2)
    assert swd[:2].tolist() == [2.0, 0.0] and mx[:2].tolist() == [3.0, 0.0] and np.isnan(swd[2]) and np.isnan(mx[2])
    assert swd.dtype == mx.dtype == np.float64
    swd, mx = sw.derived_distances(np.array([4.0]), np.array([9.0]), 1)
    assert swd.tolist() == [4.0] and mx.tolist() == [9.0]
    for p in (0, 3, 2.5):
        with pytest.raises(ValueError):
            sw.derived_distances(np.array([1.0]), np.array([1.0]), p)
    assert metrics.sliced_wasserstein_pairs is sw.sliced_wasserstein_pairs
    assert metrics.sliced_wasserstein_trajectories is sw.sliced_wasserstein_trajectories
    assert metrics.sliced_wasserstein_sweep is sw.sliced_wasserstein_sweep


# ------------------------------------------------------------------------------------------------ the C surface
def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


def header_constant(name):
    m = re.search(rf"#define {name} \(?([^\n/]+?)\)?\s*(?:/\*.*)?$", open(HEADER).read(), flags=re.M)
    return eval(m.group(1), {})


@pytest.fixture(scope="module")
def lib_path():
    from distillation_trajectories_amd.csrc.build import LIB, build
    return build() if not os.path.exists(LIB) else LIB


def test_binding_and_library_cover_the_header(lib_path):
    names = declared_functions()
    assert names == sorted(_hip.SWD_SIGNATURES)
    assert names == ["dt_swd", "dt_swd_distance", "dt_swd_distance_workspace_bytes", "dt_swd_sorted", "dt_swd_sorted_bytes",
                     "dt_swd_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    assert _hip.load(lib_path).dt_abi_version() == _hip.ABI_VERSION == 6
    for name, value in (("DT_SWD_MAX_N", engine.SWD_MAX_N), ("DT_SWD_MAX_E", engine.SWD_MAX_E), ("DT_SWD_MAX_L", engine.SWD_MAX_L),
                        ("DT_SWD_MAX_P", engine.SWD_MAX_P), ("DT_SWD_OK", engine.SWD_OK), ("DT_SWD_NONFINITE", engine.SWD_NONFINITE),
                        ("DT_SWD_SORTED_WORKSPACE_BYTES", engine.SWD_SORTED_WORKSPACE_BYTES)):
        assert header_constant(name) == value, name
    assert "dt_swd" not in open(os.path.join(ROOT, "include", "dt_hip.h")).read()       # nothing is added to dt_hip.h


def test_size_queries(lib_path):
    lib = _hip.load(lib_path)
    for P, n, L in ((1, 1, 1), (3, 7, 65), (51, 256, 512), (1 << 16, 2048, 4096)):
        assert lib.dt_swd_sorted_bytes(P, n, L) == 8 * P * L * n
        one, many = lib.dt_swd_workspace_bytes(1, n, 5, L), lib.dt_swd_workspace_bytes(P, n, 5, L)
        assert one >= 8 * L * (n + 5 + 1) and many - one == (P - 1) * 8 * L * (n + 5 + 1)
        assert lib.dt_swd_distance_workspace_bytes(P, L) == 8 * P * L
    for P, n, L in ((0, 4, 4), (65537, 4, 4), (1, 0, 4), (1, 2049, 4), (1, 4, 0), (1, 4, 4097), (-1, 4, 4)):
        assert lib.dt_swd_sorted_bytes(P, n, L) == 0
        assert lib.dt_swd_workspace_bytes(P, n, 4, L) == 0 and lib.dt_swd_workspace_bytes(P, 4, n, L) == 0


def test_argument_paths_are_clean_under_asan_and_ubsan():
    """tests/host_sanitize/swd_driver.cpp: a program of its own, host code instrumented; it needs no GPU"""
    from distillation_trajectories_amd.csrc.build import build_swd_sanitizer_driver
    exe = build_swd_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "swd host checks clean" in res.stdout, res.stdout + res.stderr


def test_engine_checks_arguments_first(lib_path):
    _hip.load(lib_path)
    X = torch.zeros(3, 4, 12)
    theta = engine.swd_directions(12, 8)
    for bad in (X.double(), X.half(), X.numpy(), None, torch.zeros(12), torch.zeros(2, 2, 2, 12), [X], torch.zeros(3, 0, 12),
                torch.zeros(3, 2049, 2), torch.zeros(3, 4, 0)):                                  # type, dtype, dims, limits
        with pytest.raises(ValueError):
            engine.device_swd(bad, X)
        with pytest.raises(ValueError):
            engine.device_swd(X, bad)
        with pytest.raises(ValueError):
            engine.device_swd_sorted(bad, theta)
    with pytest.raises(ValueError):
        engine.device_swd(X, torch.zeros(3, 4, 13))                                              # another width
    with pytest.raises(ValueError):
        engine.device_swd(X, torch.zeros(2, 4, 12))                                              # 3 states against 2
    for p in (0, 3, 2.0, True, None):
        with pytest.raises(ValueError):
            engine.device_swd(X, X, p=p)
    for L in (0, 4097, 2.0, True):
        with pytest.raises(ValueError):
            engine.device_swd(X, X, n_directions=L)
    for ws in (-1, 1.5, True):
        with pytest.raises(ValueError):
            engine.device_swd(X, X, workspace_bytes=ws)
    for d in (theta.double(), theta[0], theta.numpy(), engine.swd_directions(13, 8), "random"):
        with pytest.raises(ValueError):
            engine.device_swd(X, X, directions=d)
        with pytest.raises(ValueError):
            engine.device_swd_sorted(X, d)
    with pytest.raises(ValueError, match="on the device"):                                        # wrong device, last
        engine.device_swd(X, X)
    with pytest.raises(ValueError, match="on the device"):
        engine.device_swd(X, X[0], directions=theta, p=1, per_direction=True)
    with pytest.raises(ValueError, match="on the device"):
        engine.device_swd_sorted(X, theta)
    # a sorted side: its shape is checked, and directions other than its own are refused, before any device call
    made = engine.SwdSorted(torch.zeros(3, 8, 4, dtype=torch.float64), torch.zeros(3, dtype=torch.int32), 4, theta)
    for broken in (made._replace(n=5), made._replace(status=torch.zeros(2, dtype=torch.int32)), made._replace(sorted=torch.zeros(3, 8, 4)),
                   made._replace(directions=engine.swd_directions(12, 9)), made._replace(sorted=None)):
        with pytest.raises(ValueError, match="SwdSorted"):
            engine.device_swd(broken, X)
    with pytest.raises(ValueError, match="other directions"):
        engine.device_swd(made, X, directions=engine.swd_directions(12, 8, seed=1))
    with pytest.raises(ValueError, match="other directions"):
        engine.device_swd(made, made._replace(directions=theta.clone()))
    with pytest.raises(ValueError, match="on the device"):
        engine.device_swd(made, X)
    with pytest.raises(ValueError):
        sw.sliced_wasserstein_pairs(X, X.double())


def test_rows_are_described_in_place():
    """(problem, row) strides of trajectories, of views of them and of single sets; rows without unit stride are copied"""
    E = 12
    grid = torch.zeros(9, 8, E)
    t, P, n, width, ps, rs = engine._swd_rows(grid, "a")
    assert t is grid and (P, n, width, ps, rs) == (9, 8, E, 8 * E, E)
    odd = grid[1::2, 1::2]                                                   # every second state, the odd samples
    t, P, n, width, ps, rs = engine._swd_rows(odd, "a")
    assert t.data_ptr() == grid.data_ptr() + 4 * (8 * E + E) and (P, n, ps, rs) == (4, 4, 2 * 8 * E, 2 * E)
    shifted = torch.zeros(5 * E + 1)[1:].view(5, E)                          # aligned to a float only
    t, P, n, width, ps, rs = engine._swd_rows(shifted, "a")
    assert t.data_ptr() == shifted.data_ptr() and t.data_ptr() % 16 == 4 and (P, n, ps, rs) == (1, 5, 0, E)
    shared = torch.zeros(1, 4, E).expand(3, 4, E)                            # one set shown three times
    assert engine._swd_rows(shared, "a")[4:] == (0, E)
    turned = torch.zeros(E, 5).t()                                           # no unit stride along the row: copied
    t = engine._swd_rows(turned, "a")
    assert t[0].is_contiguous() and t[5] == E


def test_trajectory_forms_and_sweep_arguments(models):
    from distillation_trajectories_amd.config import Config
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 4
    teacher, student = models(0.1), models(0.05)
    for bad in (0, 1, -1, 2.0, True, 2049):
        with pytest.raises(ValueError):
            sw.sliced_wasserstein_sweep(teacher, [student], cfg, [1.0], bad)
    with pytest.raises(ValueError):
        sw.sliced_wasserstein_sweep(teacher, [], cfg, [1.0], 4)
    with pytest.raises(ValueError):
        sw.sliced_wasserstein_sweep(teacher, [student], cfg, [], 4)
    with pytest.raises(ValueError):
        sw.sliced_wasserstein_sweep(teacher, [student], cfg, [1.0], 4, every=0)
    with pytest.raises(ValueError):
        sw.sliced_wasserstein_sweep(teacher, [student], cfg, [1.0], 4, p=3)
    with pytest.raises(ValueError):
        sw.sliced_wasserstein_sweep(teacher, [student], cfg, [1.0], 4, n_directions=0)
    other = type("Other", (), {"image_size": 32})()
    with pytest.raises(ValueError, match="resolution"):
        sw.sliced_wasserstein_sweep(teacher, [student, other], cfg, [1.0], 4)
    a = [torch.zeros(2, 3, 4, 4) for _ in range(3)]
    with pytest.raises(ValueError, match="states"):
        sw.sliced_wasserstein_trajectories(a, a[:2])                          # unequal lengths are refused
