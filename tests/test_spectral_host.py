"""Spatial-frequency spectra without a GPU: the yardstick spectral_ref64 against numpy's FFT and Parseval, the margin a
plain float64 transform leaves under its coefficient bound, the radial table, the derived band metrics, the exported
surface of include/dt_hip_spectral.h, the workspace query, and argument checks that fail before any device call."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import spectral_ref64 as ref
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.analysis import metrics
from distillation_trajectories_amd.analysis.metrics import spectral

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dt_hip_spectral.h")
SHAPES = [(2, 2), (3, 5), (16, 16), (28, 28), (32, 32), (64, 64), (64, 7), (1, 64)]


def _kinds(seed, H, W):
    g = np.random.RandomState(seed).standard_normal((2, H, W))
    return {"gauss": g.astype(np.float32), "offset": (g + 100.0).astype(np.float32), "flat": (1.0 + 1e-3 * g).astype(np.float32)}


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("H,W", SHAPES)
def test_yardstick_equals_numpy_fft(H, W):
    """to 1e-13 sum|x| (measured: at most 1e-16 sum|x|)"""
    for x in _kinds(1, H, W).values():
        got, want = ref.dft2(x), np.fft.fft2(x.astype(np.float64))
        scale = np.abs(x.astype(np.float64)).sum(axis=(-2, -1))[:, None, None]
        assert (np.abs(got - want).astype(np.float64) <= 1e-13 * scale).all()


@pytest.mark.parametrize("H,W", SHAPES)
def test_plain_float64_transform_stays_below_a_tenth_of_delta(H, W):
    worst = 0.0
    for x in _kinds(2, H, W).values():
        err = np.abs(ref.dft2_plain64(x).astype(ref.CLD) - ref.dft2(x))
        worst = max(worst, float((err / ref.delta(x)[:, None, None]).max()))
    print(f"{H}x{W}: plain float64 error / delta = {worst:.4f}")
    assert worst < 0.10


@pytest.mark.parametrize("H,W", [(3, 5), (16, 16), (64, 7)])
def test_parseval_of_the_difference_spectrum(H, W):
    a, b = ref.pictures(3, (2, H, W), "gauss")
    table, cells = engine.radial_bins(H, W)
    sums = ref.pair_sums(a, b, table, len(cells))
    want = H * W * (ref.difference(a, b).astype(ref.LD) ** 2).sum(axis=(-2, -1))
    assert (np.abs(sums[..., ref.D].sum(axis=-1) - want) <= 1e-17 * want).all()
    assert (np.abs(ref.power_sums(a, table, len(cells)) - sums[..., ref.PA]) == 0).all()
    near = ref.pictures(4, (2, H, W), "near")
    bound = ref.forward_bound(*near, table, len(cells)).astype(np.float64)
    sums = ref.pair_sums(*near, table, len(cells)).astype(np.float64)
    has = sums[..., ref.D] > 0
    assert (bound[..., ref.D][has] < 1e-10 * sums[..., ref.D][has]).all()      # the bound follows the difference: it stays ...
    assert (bound[..., ref.D][has] < 1e-3 * bound[..., ref.PA][has]).all()     # ... far below that of the powers themselves


def test_bin_sum_leaves_out_what_the_table_leaves_out():
    table, n = ref.holes_table(3, 5)
    assert table[0, 0] == -1 and (table == -1).sum() == 4 and n == 3
    v = np.arange(15, dtype=np.float64).reshape(3, 5)
    got = ref.bin_sum(v, table, n)
    assert got.sum() == v[table >= 0].sum() and got[1] == v[table == 1].sum()
    assert ref.status(np.zeros((2, 1, 2, 2))).tolist() == [0, 0]
    bad = np.zeros((2, 1, 2, 2))
    bad[1, 0, 1, 1] = np.inf
    assert ref.status(np.zeros((2, 1, 2, 2)), bad).tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ the radial table
def test_radial_table_of_4_by_4_by_hand():
    """fu, fv = [0, 1, 2, 1]; r = sqrt(fu^2 + fv^2): 1.41 -> 1, 2.24 -> 2, 2.83 -> 3"""
    table, cells = engine.radial_bins(4, 4)
    assert table.dtype == np.int32
    assert table.tolist() == [[0, 1, 2, 1], [1, 1, 2, 1], [2, 2, 3, 2], [1, 1, 2, 1]]
    assert cells.tolist() == [1, 8, 6, 1]


@pytest.mark.parametrize("H,W", SHAPES + [(5, 3), (7, 64), (63, 64)])
def test_radial_table_properties(H, W):
    table, cells = engine.radial_bins(H, W)
    assert table.shape == (H, W) and cells.sum() == H * W and len(cells) == table.max() + 1
    assert table[0, 0] == 0 and cells[0] == 1                                                  # DC alone in bin 0
    u, v = np.arange(H), np.arange(W)
    assert np.array_equal(table, table[(-u) % H][:, (-v) % W])                                # (u, v) -> (-u, -v)
    M = max(H, W)
    r = np.hypot(np.minimum(u, H - u)[:, None] * (M / H), np.minimum(v, W - v)[None, :] * (M / W))
    off_tie = np.abs(r - np.floor(r) - 0.5) > 1e-9
    assert np.array_equal(table[off_tie], np.floor(r + 0.5).astype(np.int32)[off_tie])


def test_radial_table_sizes():
    assert len(engine.radial_bins(64, 64)[1]) == 46
    table, cells = engine.radial_bins(64, 7)
    assert len(cells) == 43 and table[0].tolist() == [0, 9, 18, 27, 27, 18, 9] and table[32, 3] == 42
    assert table[:, 0].tolist() == np.minimum(np.arange(64), 64 - np.arange(64)).tolist()
    assert np.array_equal(engine.radial_bins(7, 64)[0], table.T)
    assert engine.radial_bins(1, 1)[0].tolist() == [[0]]
    assert engine.radial_bins(2, 2)[0].tolist() == [[0, 1], [1, 1]]                           # sqrt 2 = 1.41 -> 1
    for bad in ((0, 4), (4, 65), (4.0, 4), (True, 4)):
        with pytest.raises(ValueError):
            engine.radial_bins(*bad)


# ------------------------------------------------------------------------------------------------ derived metrics
def test_derived_metrics():
    cells = np.array([1, 4, 0])
    pa = np.array([[8.0, 16.0, 0.0], [2.0, 0.0, 0.0]])
    pb = np.array([[2.0, 16.0, 0.0], [2.0, 3.0, 0.0]])
    cre = np.array([[4.0, -16.0, 0.0], [2.0, 0.0, 0.0]])
    err = np.array([[2.0, 64.0, 0.0], [0.0, 3.0, 0.0]])
    r = spectral.derived_metrics(pa, pb, cre, err, np.array([2, 1]), cells, 1, 2, 2)
    assert r["power_teacher"][0, :2].tolist() == [1.0, 0.5] and np.isnan(r["power_teacher"][0, 2])
    assert r["power_student"][1, :2].tolist() == [0.5, 0.1875]
    assert r["band_correlation"][0, :2].tolist() == [1.0, -1.0] and np.isnan(r["band_correlation"][:, 2]).all()
    assert r["relative_error"][0, :2].tolist() == [0.25, 4.0] and np.isnan(r["relative_error"][1, 1])
    want = np.sqrt(((10 * np.log10(0.25)) ** 2 + 0.0) / 2)
    assert abs(r["log_spectral_distance"][0] - want) < 1e-15 and r["log_spectral_distance"][1] == 0.0
    none = spectral.derived_metrics(pa * 0, pb, cre, err, np.array([2, 1]), cells, 1, 2, 2)
    assert np.isnan(none["log_spectral_distance"]).all()
    wide = spectral.derived_metrics(pa.astype(ref.LD), pb.astype(ref.LD), cre.astype(ref.LD), err.astype(ref.LD),
                                    np.array([2, 1]), cells, 1, 2, 2)
    assert wide["relative_error"].dtype == ref.LD
    assert metrics.spectral_pairs is spectral.spectral_pairs and metrics.spectral_sweep is spectral.spectral_sweep
    assert metrics.spectral_trajectories is spectral.spectral_trajectories


# ------------------------------------------------------------------------------------------------ the C surface
def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
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
    assert names == sorted(_hip.SPECTRAL_SIGNATURES)
    assert names == ["dt_spectral_pair", "dt_spectral_power", "dt_spectral_sum", "dt_spectral_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    assert _hip.load(lib_path).dt_abi_version() == _hip.ABI_VERSION == 6
    for name, value in (("DT_SPECTRAL_MAX_HW", engine.SPECTRAL_MAX_HW), ("DT_SPECTRAL_MAX_C", engine.SPECTRAL_MAX_C),
                        ("DT_SPECTRAL_MAX_BINS", engine.SPECTRAL_MAX_BINS), ("DT_SPECTRAL_MAX_ROWS", engine.SPECTRAL_MAX_ROWS),
                        ("DT_SPECTRAL_PAIR_K", engine.SPECTRAL_PAIR_K), ("DT_SPECTRAL_PA", engine.SPECTRAL_PA),
                        ("DT_SPECTRAL_PB", engine.SPECTRAL_PB), ("DT_SPECTRAL_CRE", engine.SPECTRAL_CRE),
                        ("DT_SPECTRAL_CIM", engine.SPECTRAL_CIM), ("DT_SPECTRAL_D", engine.SPECTRAL_D),
                        ("DT_SPECTRAL_OK", engine.SPECTRAL_OK), ("DT_SPECTRAL_NONFINITE", engine.SPECTRAL_NONFINITE)):
        assert header_constant(name) == value, name
    assert (ref.PA, ref.PB, ref.CRE, ref.CIM, ref.D) == (0, 1, 2, 3, 4)


def test_workspace_query(lib_path):
    lib = _hip.load(lib_path)
    for H, W in SHAPES:
        need = lib.dt_spectral_workspace_bytes(H, W, 1)
        assert need >= 4 * (engine.SPECTRAL_MAX_BINS + 1 + H * W) and need % 16 == 0
        assert need == lib.dt_spectral_workspace_bytes(H, W, 256)
    assert lib.dt_spectral_workspace_bytes(64, 64, 46) <= 32768                  # it does not grow with the rows
    for H, W, n in ((0, 4, 4), (65, 4, 4), (4, 0, 4), (4, 65, 4), (4, 4, 0), (4, 4, 257), (-4, 4, 4)):
        assert lib.dt_spectral_workspace_bytes(H, W, n) == 0


def test_argument_paths_are_clean_under_asan_and_ubsan():
    """tests/host_sanitize/spectral_driver.cpp: a program of its own, host code instrumented; it needs no GPU"""
    from distillation_trajectories_amd.csrc.build import build_spectral_sanitizer_driver
    exe = build_spectral_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "spectral host checks clean" in res.stdout, res.stdout + res.stderr


def test_engine_checks_arguments_first(lib_path):
    _hip.load(lib_path)
    X = torch.zeros(3, 2, 48)
    calls = (lambda x, *a, **k: engine.device_spectrum(x, *a, **k), lambda x, *a, **k: engine.device_spectral_pair(x, x, *a, **k),
             lambda x, *a, **k: engine.device_spectral_pair(X, x, *a, **k))
    for call in calls:
        for bad in (X.double(), X.half(), X.numpy(), None, torch.zeros(48), torch.zeros(2, 2, 2, 12), [X]):   # type, dtype, dims
            with pytest.raises(ValueError):
                call(bad, 3, 4, 4)
        for C, H, W in ((3, 4, 5), (1, 4, 4), (3, 2, 4), (48, 1, 2)):                                         # E != C*H*W
            with pytest.raises(ValueError):
                call(X, C, H, W)
        for C, H, W in ((0, 4, 4), (65, 4, 4), (3, 0, 4), (3, 65, 4), (3, 4, 65), (3.0, 4, 4), (3, True, 4), (3, 4, -4)):   # limits
            with pytest.raises(ValueError):
                call(torch.zeros(2, max(int(C * H * W), 1)), C, H, W)
        for bins in (np.zeros((4, 5), dtype=np.int32), np.zeros(16, dtype=np.int32), np.zeros((4, 4)), np.full((4, 4), -1),
                     np.full((4, 4), 256), np.full((4, 4), -2), torch.zeros(3, 4, dtype=torch.int32), "radial"):  # table
            with pytest.raises(ValueError):
                call(X, 3, 4, 4, bins=bins)
        for ws in (-1, 1.5, True):
            with pytest.raises(ValueError):
                call(X, 3, 4, 4, workspace_bytes=ws)
        with pytest.raises(ValueError, match="on the device"):                                                  # wrong device, last
            call(X, 3, 4, 4)
        with pytest.raises(ValueError, match="on the device"):
            call(X, 3, 4, 4, bins=np.zeros((4, 4), dtype=np.int64), sum_samples=True)
    with pytest.raises(ValueError):
        engine.device_spectral_pair(X, None, 3, 4, 4)
    with pytest.raises(ValueError):
        engine.device_spectral_pair(X, torch.zeros(3, 3, 48), 3, 4, 4)
    with pytest.raises(ValueError):
        engine.device_spectral_pair(X, torch.zeros(6, 48), 3, 4, 4)
    with pytest.raises(ValueError):
        engine.device_spectrum(torch.zeros(0, 48), 3, 4, 4)
    with pytest.raises(ValueError):
        spectral.spectral_pairs(X, X.double(), 3, 4, 4)


def test_rows_are_described_in_place():
    """(outer, inner) strides of trajectories, of views of them and of flat sets; rows without unit stride are copied"""
    E = 12
    grid = torch.zeros(9, 7, E)
    t, lead, n_outer, n_inner, ostride, istride = engine._spectral_rows(grid, "X", E)
    assert t is grid and (lead, n_outer, n_inner, ostride, istride) == ((9, 7), 9, 7, 7 * E, E)
    view = grid[1::2, 1:5]                                                  # every second state, a slice of the samples
    t, lead, n_outer, n_inner, ostride, istride = engine._spectral_rows(view, "X", E)
    assert t.data_ptr() == grid.data_ptr() + 4 * (7 * E + E) and (lead, ostride, istride) == ((4, 4), 2 * 7 * E, E)
    flat = torch.zeros(5, 2 * E)[:, E:]
    t, lead, n_outer, n_inner, ostride, istride = engine._spectral_rows(flat, "X", E)
    assert t.data_ptr() == flat.data_ptr() and (lead, n_outer, n_inner, ostride, istride) == ((5,), 1, 5, 0, 2 * E)
    spread = torch.zeros(3, 1, E).expand(3, 4, E)                           # one row shown four times
    assert engine._spectral_rows(spread, "X", E)[4:] == (E, 0)
    turned = torch.zeros(E, 5).t()                                          # no unit stride along the row: copied
    t = engine._spectral_rows(turned, "X", E)
    assert t[0].is_contiguous() and t[5] == E


def test_trajectory_forms_and_sweep_arguments(models):
    from distillation_trajectories_amd.config import Config
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 4
    teacher, student = models(0.1), models(0.05)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            spectral.spectral_sweep(teacher, [student], cfg, [1.0], bad)
    with pytest.raises(ValueError):
        spectral.spectral_sweep(teacher, [], cfg, [1.0], 4)
    with pytest.raises(ValueError):
        spectral.spectral_sweep(teacher, [student], cfg, [], 4)
    with pytest.raises(ValueError):
        spectral.spectral_sweep(teacher, [student], cfg, [1.0], 4, every=0)
    other = type("Other", (), {"image_size": 32})()
    with pytest.raises(ValueError, match="resolution"):
        spectral.spectral_sweep(teacher, [student, other], cfg, [1.0], 4)
    big = Config()
    big.image_size, big.timesteps = 128, 4
    with pytest.raises(ValueError):
        spectral.spectral_sweep(teacher, [student], big, [1.0], 4)
    assert spectral._state_view(torch.arange(7), [0, 3, 6]).tolist() == [0, 3, 6]
    assert spectral._state_view(torch.arange(8), [0, 3, 6, 7]).tolist() == [0, 3, 6, 7]
    assert spectral._state_view(torch.arange(8), [5]).tolist() == [5]
    base = torch.arange(70.0).view(7, 10)
    assert spectral._state_view(base, [0, 3, 6]).data_ptr() == base.data_ptr()            # a view, not a copy
