"""Trajectory alignment without a GPU: the yardstick align_ref64 against a brute-force minimum over every monotone path,
its tie and band rules, the exported surface of include/dt_hip_align.h, the workspace queries, argument checks that fail
before any device call, and the derived quantities of analysis/metrics/alignment.py on a hand-made path."""
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import align_ref64 as ref
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.analysis.metrics import alignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dt_hip_align.h")
SHAPES = [s for s in itertools.product(range(1, 6), repeat=2)]
KINDS = (ref.DTW, ref.FRECHET)


def _matrix(n_a, n_b, seed):
    """small random integers: sums and maxima of a few of them are exact in float64"""
    return np.random.RandomState(seed).randint(0, 10, size=(n_a, n_b)).astype(np.float64)


@pytest.mark.parametrize("kind", KINDS)
def test_yardstick_equals_brute_force_on_every_shape_up_to_5x5(kind):
    for n_a, n_b in SHAPES:
        for seed in range(4):
            D = _matrix(n_a, n_b, 100 * n_a + 10 * n_b + seed)
            value, path, status = ref.dp(D, kind)
            want = ref.brute_force(D, kind)
            assert status == ref.OK
            if kind == ref.FRECHET:
                assert value == want, (n_a, n_b, seed)
            else:
                assert abs(value - want) <= 1e-12 * abs(want), (n_a, n_b, seed)


@pytest.mark.parametrize("kind", KINDS)
def test_yardstick_path_attains_its_value(kind):
    for n_a, n_b in SHAPES:
        D = _matrix(n_a, n_b, 7 * n_a + n_b)
        value, path, _ = ref.dp(D, kind)
        assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (n_a - 1, n_b - 1)
        steps = np.diff(path, axis=0)
        assert all(tuple(s) in ((1, 1), (1, 0), (0, 1)) for s in steps)
        got = ref.path_value(D, path, kind)
        assert got == value if kind == ref.FRECHET else abs(got - value) <= 1e-12 * abs(value)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(4, 4), (3, 6), (6, 3)])
def test_ties_take_the_diagonal_then_the_straight_remainder(kind, shape):
    n_a, n_b = shape
    _, path, _ = ref.dp(np.ones(shape), kind)
    m = min(n_a, n_b)
    # walking back from the end the diagonal wins every tie until an edge is reached: the straight part comes first
    lead = [(0, j) for j in range(n_b - m)] if n_b > n_a else [(i, 0) for i in range(n_a - m)]
    off = (n_a - m, n_b - m)
    want = lead + [(off[0] + k, off[1] + k) for k in range(m)]
    assert [tuple(c) for c in path] == want


def test_band_contains_both_corners_and_is_symmetric():
    for n_a, n_b in itertools.product((2, 3, 5, 17, 64), repeat=2):
        for band in (1, 2, 4):
            allowed = ref.band_mask(n_a, n_b, band)
            assert allowed[0, 0] and allowed[-1, -1]
            assert np.array_equal(allowed, ref.band_mask(n_b, n_a, band).T)
            assert np.array_equal(allowed, allowed[::-1, ::-1])
            value, path, status = ref.dp(_matrix(n_a, n_b, band), ref.DTW, band)
            assert status == ref.OK and all(allowed[i, j] for i, j in path)   # every band >= 1 leaves a path
    assert ref.band_mask(4, 7, 0).all()
    assert np.array_equal(ref.band_mask(5, 5, 1), np.abs(np.subtract.outer(np.arange(5), np.arange(5))) <= 1)


@pytest.mark.parametrize("kind", KINDS)
def test_a_band_that_cuts_every_path_gives_no_path(kind):
    allowed = np.ones((4, 5), dtype=bool)
    allowed[:, 2] = False                                   # a forbidden column: no monotone path crosses it
    value, path, status = ref.dp(_matrix(4, 5, 3), kind, allowed=allowed)
    assert status == ref.NO_PATH and math.isinf(value) and len(path) == 0
    allowed = np.ones((4, 5), dtype=bool)
    allowed[1, 1] = allowed[0, 1] = False                   # a dent only: the path goes round it
    value, path, status = ref.dp(_matrix(4, 5, 3), kind, allowed=allowed)
    assert status == ref.OK and all(allowed[i, j] for i, j in path)


def test_non_finite_matrix_is_refused_by_the_yardstick():
    D = _matrix(3, 3, 0)
    D[1, 2] = np.nan
    value, path, status = ref.dp(D, ref.DTW)
    assert status == ref.NONFINITE and math.isnan(value) and len(path) == 0


def test_cost_matrix_of_the_yardstick():
    rs = np.random.RandomState(0)
    a, b = rs.randn(3, 5).astype(np.float32), rs.randn(4, 5).astype(np.float32)
    b[2] = a[1]
    D = ref.cost_matrix(a, b)
    assert D[1, 2] == 0.0
    want = np.sqrt(((a[:, None, :].astype(np.float64) - b[None].astype(np.float64)) ** 2).sum(-1))
    assert np.allclose(D, want, rtol=1e-14, atol=0)
    assert np.array_equal(ref.cost_matrix(b, a), D.T)


# ------------------------------------------------------------------------------------------------ the C surface
def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib_path():
    from distillation_trajectories_amd.csrc.build import LIB, build
    return build() if not os.path.exists(LIB) else LIB


def test_binding_and_library_cover_the_header(lib_path):
    names = declared_functions()
    assert names == sorted(_hip.ALIGN_SIGNATURES)
    assert names == ["dt_align", "dt_align_cost", "dt_align_dp", "dt_align_min_workspace_bytes", "dt_align_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    assert _hip.load(lib_path).dt_abi_version() == _hip.ABI_VERSION == 6


def test_workspace_queries(lib_path):
    lib = _hip.load(lib_path)
    for n_a, n_b in ((2, 2), (51, 51), (3, 129), (1024, 1024)):
        blocks = (n_a + n_b - 1 + 7) // 8
        for want_path, cost_given in itertools.product((0, 1), repeat=2):
            one = lib.dt_align_min_workspace_bytes(n_a, n_b, want_path, cost_given)
            need = (0 if cost_given else 8 * n_a * n_b) + (8 * blocks * n_a if want_path else 0)
            assert one >= max(need, 1) and one % 16 == 0 and one < need + 32
            assert lib.dt_align_workspace_bytes(7, n_a, n_b, want_path, cost_given) == 7 * one
    for bad in ((1, 5), (5, 1), (1025, 5), (5, 1025), (0, 0)):
        assert lib.dt_align_min_workspace_bytes(*bad, 1, 0) == 0
    assert lib.dt_align_workspace_bytes(0, 5, 5, 1, 0) == 0 and lib.dt_align_workspace_bytes(65536, 5, 5, 1, 0) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch(lib_path):
    """null pointers, shapes, kinds, bands and workspaces: each returns its DT_E_* code (no device is needed to get there)"""
    lib = _hip.load(lib_path)
    x = torch.zeros(64, dtype=torch.float64)
    p = x.data_ptr()
    rows = (p, 4, 0, 4, p, 4, 0, 4)
    assert lib.dt_align_cost(None, 4, 0, 4, p, 4, 0, 4, 1, 4, p, p, None) == -1
    assert lib.dt_align_cost(p, 1, 0, 4, p, 4, 0, 4, 1, 4, p, p, None) == -2
    assert lib.dt_align_cost(p, 4, 0, 4, p, 1025, 0, 4, 1, 4, p, p, None) == -2
    assert lib.dt_align_cost(*rows, 1, 0, p, p, None) == -2
    assert lib.dt_align_cost(*rows, 0, 4, p, p, None) == -2
    assert lib.dt_align_dp(None, 1, 2, 2, 0, 0, p, None, None, p, p, 64, None) == -1
    assert lib.dt_align_dp(p, 1, 2, 2, 0, 0, p, p, None, p, p, 64, None) == -1       # a path without its length
    assert lib.dt_align_dp(p, 1, 1, 2, 0, 0, p, None, None, p, p, 64, None) == -2
    assert lib.dt_align_dp(p, 1, 2, 2, 2, 0, p, None, None, p, p, 64, None) == -3    # kind
    assert lib.dt_align_dp(p, 1, 2, 2, 0, -1, p, None, None, p, p, 64, None) == -3   # band
    assert lib.dt_align_dp(p, 1, 2, 2, 0, 0, p, p, p, p, p, 8, None) == -4
    tail = (None, p, p, None, None, None, None, p, p)
    assert lib.dt_align(*rows, 1, 4, 0, 0, *tail, 512, None) == -3                   # no kind asked for
    assert lib.dt_align(*rows, 1, 4, 1, 0, None, None, p, None, None, None, None, p, p, 512, None) == -1   # DTW without its output
    assert lib.dt_align(*rows, 1, 4, 2, 0, None, p, p, p, p, None, None, p, p, 512, None) == -3   # a DTW path, no DTW
    assert lib.dt_align(*rows, 1, 4, 3, 0, *tail, 8, None) == -4
    assert lib.dt_align(p, 1025, 0, 4, p, 4, 0, 4, 1, 4, 3, 0, *tail, 512, None) == -2


def test_argument_paths_are_clean_under_asan_and_ubsan():
    """tests/host_sanitize/align_driver.cpp: a program of its own, host code instrumented; it needs no GPU"""
    from distillation_trajectories_amd.csrc.build import build_align_sanitizer_driver
    exe = build_align_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "align host checks clean" in res.stdout, res.stdout + res.stderr


def test_engine_checks_arguments_first_and_refuses_cpu_tensors(lib_path):
    _hip.load(lib_path)
    X, Y = torch.zeros(4, 2, 6), torch.zeros(5, 2, 6)
    for kw in (dict(kind="soft"), dict(band=-1), dict(band=1.5), dict(layout="rows"), dict(workspace_bytes=8)):
        with pytest.raises(ValueError):
            engine.device_align(X, Y, **kw)
    for bad_x, bad_y in ((torch.zeros(1, 2, 6), Y), (torch.zeros(1025, 1, 2), torch.zeros(3, 1, 2)), (X, torch.zeros(5, 3, 6)),
                         (X, torch.zeros(5, 2, 7)), (X.double(), Y), (X.numpy(), Y)):
        with pytest.raises(ValueError):
            engine.device_align(bad_x, bad_y)
    with pytest.raises(ValueError):
        engine.device_align_cost(torch.zeros(1, 1, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        engine.device_align_cost(torch.zeros(1, 4, 4))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        engine.device_align(X, Y)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        engine.device_align_cost(torch.zeros(1, 4, 4, dtype=torch.float64))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        engine.device_align_cost_matrix(X, Y)


def test_rows_are_used_in_place():
    """step-major [n, S, C, H, W] and problem-major [P, n, E] both become [n, P, E] views of the same storage"""
    X = torch.zeros(4, 3, 2, 2, 2)
    v = engine._align_rows(X, "X", "step")
    assert tuple(v.shape) == (4, 3, 8) and v.data_ptr() == X.data_ptr() and v.stride() == (24, 8, 1)
    Xp = torch.zeros(3, 4, 8)
    v = engine._align_rows(Xp, "X", "problem")
    assert tuple(v.shape) == (4, 3, 8) and v.data_ptr() == Xp.data_ptr() and v.stride() == (8, 32, 1)
    v = engine._align_rows(torch.zeros(5, 7), "X", "step")
    assert tuple(v.shape) == (5, 1, 7)
    sl = torch.zeros(6, 3, 16)[::2, :, 3:12]
    v = engine._align_rows(sl, "X", "step")
    assert v.data_ptr() == sl.data_ptr() and v.stride() == (96, 16, 1)


# ------------------------------------------------------------------------------------------------ derived quantities
def test_path_summary_on_a_hand_made_path():
    path = [(0, 0), (1, 0), (2, 1), (2, 2), (3, 2), (4, 2)]          # 5 teacher steps, 3 student steps
    s = alignment.path_summary(path, 5, 3)
    dev = [0.0, 0.25, 0.0, 0.5, 0.25, 0.0]
    assert s["warp_deviation_max"] == 0.5
    assert s["warp_deviation_mean"] == pytest.approx(sum(dev) / 6, rel=1e-15)
    assert np.array_equal(s["teacher_to_student"], [0.0, 0.0, 1.5, 2.0, 2.0])
    straight = alignment.path_summary([(k, k) for k in range(4)], 4, 4)
    assert straight["warp_deviation_max"] == 0.0 and np.array_equal(straight["teacher_to_student"], np.arange(4.0))
    empty = alignment.path_summary(np.zeros((0, 2)), 4, 3)
    assert math.isnan(empty["warp_deviation_mean"]) and np.isnan(empty["teacher_to_student"]).all()


def test_pair_result_from_host_arrays():
    host = {"dtw": np.array([6.0]), "frechet": np.array([2.0]), "status": np.array([0], dtype=np.int32),
            "dtw_path": np.array([[[0, 0], [1, 1], [2, 1], [-1, -1]]], dtype=np.int32), "dtw_path_len": np.array([3]),
            "frechet_path": np.array([[[0, 0], [1, 0], [2, 1], [-1, -1]]], dtype=np.int32), "frechet_path_len": np.array([3])}
    r = alignment._pair_result(host, 0, 3, 2, False)
    assert r["dtw_distance"] == 6.0 and r["dtw_normalized"] == 2.0 and r["frechet_distance"] == 2.0
    assert r["dtw_path"].shape == (3, 2) and r["frechet_path"].shape == (3, 2) and "cost_matrix" not in r
    assert r["warp_deviation_max"] == 0.5 and np.array_equal(r["teacher_to_student"], [0.0, 1.0, 1.0])
    from distillation_trajectories_amd.analysis import metrics
    assert metrics.align_trajectories is alignment.align_trajectories and metrics.alignment_sweep is alignment.alignment_sweep
