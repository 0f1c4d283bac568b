"""The device PCA without a GPU: the float64 yardstick against sklearn, the reference's own (randomized) call against the
yardstick, the exported surface of include/dt_hip_pca.h, the import surface through the reference's module names, and
argument checks that fail before any device call."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from distillation_trajectories_amd import _hip
from pca_ref64 import pca_ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = range(4)


def _pair_rows(golden, i):
    arrays, _ = golden
    t, s = arrays[f"pair{i}_teacher"], arrays[f"pair{i}_student"]
    return np.vstack([t.reshape(len(t), -1), s.reshape(len(s), -1)])          # fp32 [102, 768], teacher rows first


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_ref64_equals_sklearn_full_solver(golden):
    PCA = pytest.importorskip("sklearn.decomposition").PCA
    for i in PAIRS:
        X = _pair_rows(golden, i).astype(np.float64)
        for k in (2, 3):
            sk = PCA(n_components=k, svd_solver="full").fit(X)
            ref = pca_ref64(X, k)
            assert _rel(ref["mean"], sk.mean_) < 1e-10
            assert _rel(ref["components"], sk.components_) < 1e-10, (i, k)
            assert _rel(ref["scores"], sk.transform(X)) < 1e-10, (i, k)
            for name in ("singular_values", "explained_variance", "explained_variance_ratio"):
                assert _rel(ref[name], getattr(sk, name + "_")) < 1e-10, (i, k, name)


def test_reference_randomized_call_is_within_1e4_of_ref64(golden):
    """The reference runs PCA(2|3) on the fp32 rows; sklearn picks the randomized solver for these shapes and the
    reference gives it no random_state, so its output varies from run to run.  It stays within 1e-4 relative of the
    exact PCA, which is why the device is compared with pca_ref64 and not with the reference's run."""
    PCA = pytest.importorskip("sklearn.decomposition").PCA
    for i in PAIRS:
        X = _pair_rows(golden, i)
        for k in (2, 3):
            pca = PCA(n_components=k)
            got = pca.fit_transform(X)
            ref = pca_ref64(X, k)
            for j in range(k):
                # the randomized solver's sign follows the same svd_flip rule
                assert _rel(got[:, j], ref["scores"][:, j]) < 1e-4, (i, k, j)
            assert _rel(pca.explained_variance_ratio_, ref["explained_variance_ratio"]) < 1e-4


def _pca_header_functions():
    text = open(os.path.join(ROOT, "include", "dt_hip_pca.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_exports_agree():
    from distillation_trajectories_amd.csrc.build import LIB, build
    path = build() if not os.path.exists(LIB) else LIB
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    names = _pca_header_functions()
    assert names == ["dt_pca_fit", "dt_pca_project", "dt_pca_workspace_bytes"]
    assert sorted(_hip.PCA_SIGNATURES) == names
    assert set(names) <= exported
    others = set(_hip.SIGNATURES) | set(_hip.NOISE_SIGNATURES) | set(_hip.INCEPTION_SIGNATURES)
    assert not set(names) & others
    lib = _hip.load(path)
    assert lib.dt_abi_version() == _hip.ABI_VERSION == 6
    assert all(getattr(lib, n).argtypes is not None for n in names)


def test_workspace_query_rejects_shapes_outside_the_limits():
    lib = _hip.load()
    assert lib.dt_pca_workspace_bytes(256, 202, 3072, 2) > 256 * 202 * 202 * 8
    for args in ((0, 10, 8, 2), (1, 1, 8, 1), (1, 10, 6, 2), (1, 10, 8, 0), (1, 10, 8, 10), (1, 40, 64, 17),
                 (1, 10, 4, 5)):
        assert lib.dt_pca_workspace_bytes(*args) == 0, args


def test_sanitizer_driver_covers_every_pca_entry():
    """tests/host_sanitize/pca_driver.cpp calls every function include/dt_hip_pca.h declares."""
    src = open(os.path.join(ROOT, "tests", "host_sanitize", "pca_driver.cpp")).read()
    missing = [n for n in _pca_header_functions() if n + "(" not in src]
    assert not missing, missing


def test_reference_names_import_after_aliases():
    import distillation_trajectories_amd as pkg
    from distillation_trajectories_amd.analysis.dimensionality import dimensionality_reduction as dr
    from distillation_trajectories_amd.analysis.dimensionality import latent_space as ls
    pkg.remove_aliases()
    try:
        pkg.install_aliases()
        from analysis.dimensionality.dimensionality_reduction import dimensionality_reduction_analysis
        from analysis.dimensionality.latent_space import generate_latent_space_visualization
        assert dimensionality_reduction_analysis is dr.dimensionality_reduction_analysis
        assert generate_latent_space_visualization is ls.generate_latent_space_visualization
    finally:
        pkg.remove_aliases()


def test_bad_arguments_raise_before_any_device_call(monkeypatch):
    from distillation_trajectories_amd import engine

    def no_load(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_hip, "load", no_load)
    a = torch.zeros(5, 3, 8)
    for k in (0, 5, 17, 2.0, True):                 # k <= min(16, n - 1, E) with n = 5
        with pytest.raises(ValueError, match="n_components"):
            engine.device_pca(a, k)
    with pytest.raises(ValueError, match="n >= 2"):
        engine.device_pca(torch.zeros(1, 3, 8), 1)
    with pytest.raises(ValueError, match="does not match"):
        engine.device_pca(a, 2, torch.zeros(4, 3, 12))
    with pytest.raises(ValueError, match="does not match"):
        engine.device_pca(a, 2, torch.zeros(4, 2, 8))
    with pytest.raises(ValueError, match="float32"):
        engine.device_pca(a.double(), 2)
    with pytest.raises(ValueError, match="not match"):
        engine.device_pca_project(a, torch.zeros(8), torch.zeros(2, 7))
    from distillation_trajectories_amd.analysis.dimensionality.pca import TrajectoryPCA
    with pytest.raises(ValueError):
        TrajectoryPCA(4).fit(np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError):
        TrajectoryPCA(2).transform(np.zeros((3, 8), np.float32))
