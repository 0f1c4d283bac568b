"""The device PCA without a GPU: the float64 yardstick against sklearn, the reference's own (randomized) call against the
yardstick, the exported surface of include/dt_hip_pca.h, the import surface through the reference's module names, and
argument checks that fail before any device call; the edge cases of tests/pca_cases.py (their stated spectra, the
preconditions of the comparers) and the comparers themselves, on right and on wrong answers."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from distillation_trajectories_amd import _hip
import pca_cases as pc
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


# ---------------------------------------------------------------------------------------------- the edge cases
ALL_CASES = pc.CASES + ("pairs12", "walk12")


def _f32(answer):
    """the answer as the library returns it: mean, components and scores rounded to fp32"""
    return {f: (v.astype(np.float32) if f in ("mean", "components", "scores") else v) for f, v in answer.items()}


def _resign(answer, rows, j):
    """the sign rule on component j, its score column following"""
    c = answer["components"][j]
    if c[np.argmax(np.abs(c))] < 0:
        answer["components"][j], answer["scores"][:, j] = -c, -answer["scores"][:, j]


@pytest.mark.parametrize("name", ALL_CASES)
def test_case_has_its_stated_spectrum_and_meets_the_preconditions(name):
    c = pc.case(name)
    rows, k, ref = c["rows"], c["k"], c["ref"]
    n, E = rows.shape
    assert rows.dtype == np.float32 and not rows.flags.writeable and 1 <= k <= min(16, n - 1, E) and E % 4 == 0
    pc.check_preconditions(ref, k)
    lam = pc.spectrum(ref)
    if name in pc.STATED:
        want = np.array(pc.STATED[name], np.float64)
        assert np.abs(lam[:len(want)] - want).max() <= 1e-13 * want[0], lam
    shapes = {"n2": (2, 8, 1), "n2_split": (2, 8, 1), "n3": (3, 8, 2), "n4": (4, 8, 3), "e4": (40, 4, 4), "k1": (20, 16, 1),
              "offset": (30, 16, 3), "pairs": (6, 16, 3), "stalled": (8, 16, 3), "identity_k4": (12, 12, 4),
              "identity_k11": (12, 12, 11), "rank1": (12, 16, 3), "three_points": (15, 16, 4), "near": (24, 16, 4),
              "big": (20, 16, 3), "small": (20, 16, 3), "pairs12": (12, 16, 3), "walk12": (12, 16, 3)}
    assert (n, E, k) == shapes[name]
    nulls = {"rank1": [1, 2], "three_points": [2, 3]}
    assert pc.null_directions(ref, k) == nulls.get(name, [])


def test_cases_are_what_their_names_say():
    X = pc.case("offset")["rows"].astype(np.float64)
    assert np.array_equal(X.mean(0), X.mean(0).astype(np.float32)) and abs(X.mean() - 1e4) < 1 and (X.std(0) < 0.2).all()
    for name, m in (("pairs", np.full(16, 7.0)), ("stalled", np.arange(16) % 5 + 2.0)):
        X = pc.case(name)["rows"].astype(np.float64)
        assert np.array_equal(X.mean(0), m) and np.array_equal(X, np.round(X))
    Xc = pc.case("stalled")["rows"].astype(np.float64) - (np.arange(16) % 5 + 2.0)
    assert not Xc[:2].any() and Xc[2:].any(1).all()                       # two centred rows are exactly zero
    G = (pc.case("pairs")["rows"].astype(np.float64) - 7) @ (pc.case("pairs")["rows"].astype(np.float64) - 7).T
    assert not G[np.abs(np.subtract.outer(np.arange(6) // 2, np.arange(6) // 2)) > 0].any()      # block diagonal
    X = pc.case("three_points")["rows"].astype(np.float64)
    assert len(np.unique(X, axis=0)) == 3 and np.array_equal(X.mean(0), np.round(X.mean(0))) and np.array_equal(X[:3], X[12:])
    lam = pc.spectrum(pc.case("near")["ref"])
    assert np.abs(lam[:6] / lam[0] - np.array(pc.NEAR_LAMBDA)).max() <= 1e-6 and lam[6] <= 1e-12 * lam[0]
    assert [pc.clusters(lam)[i] for i in range(3)] == [[0, 1, 2], [3], [4]]
    for name, scale in (("big", 2.0 ** 40), ("small", 2.0 ** -40)):
        X = pc.case(name)["rows"]
        assert 1.0 < np.abs(X).max() / scale < 100.0 and np.isfinite(X).all()
    assert pc.case("n2_split")["split"] == 1
    assert np.array_equal(pc.case("pairs12")["rows"][:6], pc.case("pairs")["rows"])


@pytest.mark.parametrize("name", ALL_CASES)
def test_comparer_accepts_the_reference_answer(name):
    """in float64, and rounded to fp32 as the library returns it: the bounds are attainable on every case"""
    c = pc.case(name)
    answer = pc.reference_answer(c["ref"], c["k"])
    fig = pc.compare(answer, c["rows"], c["ref"], c["k"], name)
    assert max(fig.values()) <= 1e-12, fig
    pc.compare(_f32(answer), c["rows"], c["ref"], c["k"], name)
    if name in pc.SEPARATED:
        pc.compare_vectors(_f32(answer), c["ref"], c["k"], name)


@pytest.mark.parametrize("name,members", [("pairs", [0, 1]), ("stalled", [0, 1]), ("identity_k4", list(range(11))),
                                          ("identity_k11", list(range(11))), ("near", [0, 1, 2])])
def test_comparer_accepts_a_rotated_basis_of_a_repeated_cluster(name, members):
    c = pc.case(name)
    rows, k, ref = c["rows"], c["k"], c["ref"]
    answer = pc.reference_answer(ref, k)
    Q = np.linalg.qr(np.random.RandomState(7).standard_normal((len(members), len(members))))[0]
    mixed = Q @ ref["basis"][members]                                      # another orthonormal basis of the same span
    centred = rows.astype(np.float64) - ref["mean"]
    for j in (j for j in members if j < k):
        answer["components"][j], answer["scores"][:, j] = mixed[j], centred @ mixed[j]
        _resign(answer, rows, j)
    assert not pc.close(answer["components"][0], ref["components"][0], 1e-2)
    pc.compare(_f32(answer), rows, ref, k, name)
    with pytest.raises(AssertionError):
        pc.compare_vectors(_f32(answer), ref, k, name)                     # the old comparison is wrong here


@pytest.mark.parametrize("name", ["pairs", "identity_k4", "three_points", "near", "walk12"])
def test_comparer_rejects_wrong_answers(name):
    c = pc.case(name)
    rows, k, ref = c["rows"], c["k"], c["ref"]
    lam = pc.spectrum(ref)
    right = pc.reference_answer(ref, k)
    members = pc.clusters(lam)[0]
    outside = ref["basis"][members[-1] + 1]                                # a unit vector outside component 0's cluster

    def wrong(change):
        answer = {f: v.copy() for f, v in right.items()}
        change(answer)
        return _f32(answer)

    def mix(a):
        a["components"][0] += 1e-4 * outside
    with pytest.raises(AssertionError, match="containment"):
        pc.compare(wrong(mix), rows, ref, k)

    def scale(a):
        a["components"][0] *= 1 + 1e-5
        a["scores"][:, 0] *= 1 + 1e-5                                      # consistent with it: only its length is wrong
    with pytest.raises(AssertionError, match="orthonormality" if len(members) > 1 else "component"):
        pc.compare(wrong(scale), rows, ref, k)

    def negate(a):
        a["scores"][:, 0] *= -1
    with pytest.raises(AssertionError, match="consistency"):
        pc.compare(wrong(negate), rows, ref, k)

    dead = pc.null_directions(ref, k)
    if dead:
        def noise(a):
            a["components"][dead[0]] = 7e-9 * ref["components"][dead[0]]
        with pytest.raises(AssertionError, match="null direction"):
            pc.compare(wrong(noise), rows, ref, k)

        def noisy_scores(a):
            a["scores"][:, dead[0]] = 1e-12
        with pytest.raises(AssertionError, match="null direction"):
            pc.compare(wrong(noisy_scores), rows, ref, k)

        def noisy_variance(a):
            a["explained_variance"][dead[-1]] = 1e-30
            a["singular_values"][dead[-1]] = np.sqrt(1e-30 * (len(rows) - 1))
        with pytest.raises(AssertionError, match="null direction"):
            pc.compare(wrong(noisy_variance), rows, ref, k)
