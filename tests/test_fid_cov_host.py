"""The feature-space route of the device Fréchet distance without a GPU (include/dt_hip_fid_cov.h, engine.device_fid_cov,
engine.fid_route, engine.device_fid_auto): the exported surface, the workspace query at its limits and at its largest
shape, argument checks that fail before any device call, the choice of route and which entry the drivers reach, the import
surface through the reference's module names, and the resources of the new kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from distillation_trajectories_amd import _hip, engine
from fid_ref64 import feature_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dt_hip_fid_cov.h")


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


def _lib_path():
    from distillation_trajectories_amd.csrc.build import LIB, build
    return build() if not os.path.exists(LIB) else LIB


def test_header_binding_and_exports_agree():
    path = _lib_path()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    names = _declared()
    assert names == ["dt_fid_cov_distance", "dt_fid_cov_workspace_bytes"]
    assert sorted(_hip.FID_COV_SIGNATURES) == names and set(names) <= exported
    assert not set(names) & set(_hip.FID_SIGNATURES)
    lib = _hip.load(path)
    assert lib.dt_abi_version() == _hip.ABI_VERSION == 6
    assert all(getattr(lib, n).argtypes is not None for n in names)
    assert _hip.FID_COV_SIGNATURES["dt_fid_cov_distance"] == _hip.FID_SIGNATURES["dt_fid_distance"]    # one argument list
    text = open(HEADER).read()
    for macro, value in (("DT_FID_COV_MAX_ROWS", engine.FID_COV_MAX_ROWS), ("DT_FID_COV_MAX_WIDTH", engine.FID_COV_MAX_WIDTH),
                         ("DT_FID_COV_EVENTS", engine.FID_COV_EVENTS)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value
    from distillation_trajectories_amd.csrc import build
    assert any(h.endswith("dt_hip_fid_cov.h") for h in build.HEADERS)


def _documented_bytes(P, n_a, n_b, D, slabs):
    """what the header says the query returns, with `slabs` extra matrices for the row slabs of the two products"""
    chunks = -(-n_a // 1024) + -(-n_b // 1024)
    per = (3 + slabs) * D * D + (2 * chunks + 10) * D + 16
    return P * per * 8 + -(-4 * P // 256) * 256


def test_workspace_query_rejects_shapes_outside_the_limits():
    q = _hip.load(_lib_path()).dt_fid_cov_workspace_bytes
    for args in ((0, 50, 50, 2048), (65536, 50, 50, 2048), (1, 1, 50, 2048), (1, 50, 1, 2048), (1, 131073, 50, 2048),
                 (1, 50, 131073, 2048), (1, 50, 50, 2052), (1, 50, 50, 2046), (1, 50, 50, 0), (1, 50, 50, 2),
                 (1, -3, 50, 2048), (1, 50, 50, -4)):
        assert q(*args) == 0, args


def test_workspace_query_inside_the_limits():
    q = _hip.load(_lib_path()).dt_fid_cov_workspace_bytes
    # n is not tied to D; the sample-space route's refused shape; the largest rows; the smallest of everything
    for P, n_a, n_b, D in ((1, 50, 50, 2048), (1, 2049, 2049, 2048), (11, 50000, 50000, 2048), (1, 131072, 2, 64),
                           (3, 2, 2, 4), (65535, 2, 2, 4), (2, 2500, 2300, 64), (1, 10000, 300, 512), (1, 5, 7, 1024)):
        got = q(P, n_a, n_b, D)
        assert got >= _documented_bytes(P, n_a, n_b, D, 0) > 0, (P, n_a, n_b, D, got)
        most = 0 if D >= 1024 else 16                  # up to 8 slabs per set below D = 1024, none from there up
        assert got <= _documented_bytes(P, n_a, n_b, D, most), (P, n_a, n_b, D, got)
    assert q(1, 2500, 2300, 64) == _documented_bytes(1, 2500, 2300, 64, 10)         # five slabs of 512 rows a set
    assert q(1, 300, 257, 64) == _documented_bytes(1, 300, 257, 64, 0)              # one slab: written in place
    assert q(3, 50, 60, 64) - q(2, 50, 60, 64) == _documented_bytes(1, 50, 60, 64, 0) - 256


def test_workspace_query_does_not_overflow_at_the_largest_shape():
    q = _hip.load(_lib_path()).dt_fid_cov_workspace_bytes
    got = q(65535, 131072, 131072, 2048)
    need = _documented_bytes(65535, 131072, 131072, 2048, 0)
    assert need > 65535 * 3 * 2048 * 2048 * 8 > 2 ** 42
    assert got == need, (got, need)


def test_bad_arguments_raise_before_any_device_call(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_hip, "load", no_load)
    a = torch.zeros(5, 16)
    for fn in (engine.device_fid_cov, engine.device_fid_auto):
        with pytest.raises(ValueError, match="float32"):
            fn(a.double(), a)
        with pytest.raises(ValueError, match="float32"):
            fn(a, a.half())
        with pytest.raises(ValueError, match="torch tensor"):
            fn(a.numpy(), a)
        with pytest.raises(ValueError, match=r"\[n, D\] or \[P, n, D\]"):
            fn(torch.zeros(16), a)
        with pytest.raises(ValueError, match="same feature width"):
            fn(a, torch.zeros(5, 20))
        with pytest.raises(ValueError, match="same number of problems"):
            fn(torch.zeros(3, 5, 16), torch.zeros(2, 5, 16))
        with pytest.raises(ValueError, match="at least 2 samples"):
            fn(a[:1], a)
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(torch.zeros(5, 18), torch.zeros(5, 18))
        with pytest.raises(engine.HipLibraryError, match="CUDA"):         # well-formed, but not on the device
            fn(a, a)
    # the route's own limits and its own message
    with pytest.raises(ValueError, match="feature-space.*131072.*2048"):
        engine.device_fid_cov(torch.zeros(131073, 4), a[:, :4])
    with pytest.raises(ValueError, match="feature-space.*131072.*2048"):
        engine.device_fid_cov(torch.zeros(5, 2052), torch.zeros(5, 2052))
    with pytest.raises(ValueError, match="events"):
        engine.device_fid_cov(a, a, events=[None] * 5)                    # the sample-space route's count
    with pytest.raises(engine.HipLibraryError, match="CUDA"):             # what device_fid refuses, this route takes
        engine.device_fid_cov(torch.zeros(2049, 4), torch.zeros(2049, 4))
    with pytest.raises(ValueError, match="2048.*feature-space"):          # ... and device_fid still refuses, in its words
        engine.device_fid(torch.zeros(2049, 4), torch.zeros(2049, 4))
    with pytest.raises(ValueError, match=r"min\(n_a, n_b\) <= 2048.*D <= 2048"):
        engine.device_fid_auto(torch.zeros(2049, 2052), torch.zeros(2049, 2052))


def test_fid_route_on_both_sides_of_each_threshold():
    assert engine.fid_route(2048, 9999, 2048) == "samples" and engine.fid_route(9999, 2048, 2048) == "samples"
    assert engine.fid_route(2049, 2049, 2048) == "features" and engine.fid_route(50000, 2049, 64) == "features"
    assert engine.fid_route(2048, 2048, 4096) == "samples" and engine.fid_route(50, 50, 1 << 20) == "samples"
    assert engine.fid_route(2048, 2049, 2048) == "samples" and engine.fid_route(2049, 2050, 2048) == "features"
    with pytest.raises(ValueError, match="2048.*2048"):
        engine.fid_route(2049, 2049, 4096)
    with pytest.raises(ValueError, match=r"min\(n_a, n_b\) <= 2048.*D <= 2048"):
        engine.fid_route(2049, 2049, 2052)


class _Reached(Exception):
    pass


def _patch_routes(monkeypatch):
    """both engine entries replaced by recorders; returns the list they append (name, shapes) to"""
    seen = []

    def recorder(name):
        def fn(a, b, events=None, workspace=None):
            seen.append((name, tuple(a.shape), tuple(b.shape)))
            P = b.shape[0] if b.dim() == 3 else 1
            return {"fid": torch.full((P,), 1.5, dtype=torch.float64), "parts": torch.zeros(P, 4, dtype=torch.float64),
                    "status": torch.zeros(P, dtype=torch.int32)}
        return fn
    monkeypatch.setattr(engine, "device_fid", recorder("samples"))
    monkeypatch.setattr(engine, "device_fid_cov", recorder("features"))
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)      # no device to upload to here
    return seen


def test_calculate_fid_device_reaches_the_entry_fid_route_names(monkeypatch):
    from distillation_trajectories_amd.analysis.metrics import fid_score
    seen = _patch_routes(monkeypatch)
    small, edge, big = np.zeros((50, 8), np.float32), np.zeros((2048, 8), np.float32), np.zeros((2049, 8), np.float32)
    assert fid_score.calculate_fid_device(small, big) == 1.5
    assert fid_score.calculate_fid_device(big, edge) == 1.5
    assert fid_score.calculate_fid_device(big, big) == 1.5
    assert seen == [("samples", (50, 8), (2049, 8)), ("samples", (2049, 8), (2048, 8)), ("features", (2049, 8), (2049, 8))]


@pytest.mark.parametrize("num_samples,route", [(6, "samples"), (2048, "samples"), (2049, "features")])
def test_fid_sweep_reaches_the_entry_fid_route_names(monkeypatch, num_samples, route):
    from distillation_trajectories_amd.analysis.metrics import fid_score
    seen = _patch_routes(monkeypatch)
    monkeypatch.setattr(fid_score, "generate_samples",
                        lambda model, config, n, device, fixed_samples=None: torch.zeros(n, 3, 4, 4))
    monkeypatch.setattr(fid_score, "InceptionModel", lambda device, weights=None: None)
    monkeypatch.setattr(fid_score, "extract_features", lambda samples, model, **k: torch.zeros(len(samples), 8))
    model = torch.nn.Linear(2, 2)
    res = fid_score.fid_sweep(model, [model, model], None, num_samples)
    assert seen == [(route, (num_samples, 8), (2, num_samples, 8))]
    assert res["fid"].tolist() == [1.5, 1.5] and res["status"].tolist() == [0, 0]


def test_new_names_import_after_aliases():
    import distillation_trajectories_amd as pkg
    from distillation_trajectories_amd.analysis.metrics import fid_score as fs
    pkg.remove_aliases()
    try:
        pkg.install_aliases()
        from analysis.metrics.fid_score import calculate_fid_device, fid_sweep
        assert calculate_fid_device is fs.calculate_fid_device and fid_sweep is fs.fid_sweep
        for name in ("device_fid_cov", "device_fid_auto", "fid_route", "FID_COV_EVENTS", "FID_COV_MAX_ROWS"):
            assert getattr(fs.engine, name) is getattr(engine, name), name
    finally:
        pkg.remove_aliases()


def test_feature_space_kernels_neither_spill_nor_use_scratch():
    from distillation_trajectories_amd.csrc import build
    try:
        build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.kernel_resources("dt_fid.hip")
    mine = {name: r for name, r in res.items() if name.startswith("cov_")}
    assert sorted(mine) == ["cov_chol_diag_kernel", "cov_chol_panel_kernel", "cov_chol_update_kernel", "cov_coldev_kernel",
                            "cov_colsum_kernel", "cov_cross_kernel", "cov_gram_kernel", "cov_slab_sum_kernel",
                            "cov_square_kernel", "cov_stats_kernel", "cov_tol_kernel"], sorted(res)
    for name, r in mine.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes"] == 0, (name, r)
        assert r["lds_bytes"] <= 64 * 1024, (name, r)


def test_feature_like_inputs_of_the_device_tests_are_what_they_claim():
    """the shapes with n < D have singular covariances (pivots must drop); the others are full rank"""
    for n, D, singular in ((65, 80, True), (64, 80, True), (5, 4, False), (300, 64, False), (63, 36, False)):
        a = feature_like(1000 + n, n, D).astype(np.float64)
        rank = np.linalg.matrix_rank(a - a.mean(axis=0))
        assert (rank < D) == singular, (n, D, rank)
