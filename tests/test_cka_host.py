"""Layer-wise CKA without a GPU: the yardstick cka_ref64 against the explicit H K H form and the brute-force fourth-order
U-statistic, its invariances, the conditions that keep the tolerances of tests/test_hip_cka.py honest on the shared
cases, the exported surface of include/dt_hip_cka.h, the workspace queries, and argument checks that fail before any
device call."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cka_cases
import cka_ref64 as ref
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.analysis import metrics
from distillation_trajectories_amd.analysis.metrics import representation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dt_hip_cka.h")
LD = np.longdouble


def _features(seed, n, p, offset=0.0):
    return (np.random.RandomState(seed).standard_normal((n, p)) + offset).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the yardstick
def test_biased_score_equals_the_explicit_hkh_form():
    X, Y = _features(0, 9, 5, 1.5), _features(1, 9, 12, -0.5)
    Kc, Lc = ref.centre_gram(ref.gram(X.astype(LD))), ref.centre_gram(ref.gram(Y.astype(LD)))
    want = np.trace(Kc @ Lc) / np.sqrt(np.trace(Kc @ Kc) * np.trace(Lc @ Lc))
    got = ref.cka_biased(ref.centred_gram(X), ref.centred_gram(Y))
    assert abs(float(got - want)) < 1e-15


@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_debiased_hsic_equals_the_brute_force_u_statistic(n):
    X, Y = _features(10 + n, n, 3, 0.7), _features(20 + n, n, 6)
    for K, L in ((ref.gram(X.astype(LD)), ref.gram(Y.astype(LD))), (ref.centred_gram(X), ref.centred_gram(Y)),
                 (ref.centred_gram(X), ref.centred_gram(X))):
        got, want = ref.hsic1(K, L), ref.hsic1_brute_force(K, L)
        assert abs(float(got - want)) <= 1e-16 * float(ref.inner(K, K) * ref.inner(L, L)) ** 0.5


def test_both_estimators_are_invariant_to_feature_centring():
    """HKH is the centred Gram, and HSIC1 of raw Grams equals HSIC1 of feature-centred ones: the kernel may centre first"""
    X, Y = _features(2, 11, 7, 3.0), _features(3, 11, 4, -2.0)
    raw_k, raw_l = ref.gram(X.astype(LD)), ref.gram(Y.astype(LD))
    cen_k, cen_l = ref.centred_gram(X), ref.centred_gram(Y)
    assert abs(float(ref.cka_biased(ref.centre_gram(raw_k), ref.centre_gram(raw_l)) - ref.cka_biased(cen_k, cen_l))) < 1e-14
    assert abs(float(ref.cka_unbiased(raw_k, raw_l) - ref.cka_unbiased(cen_k, cen_l))) < 1e-13
    shifted = ref.gram(ref.centred(X, means=np.zeros(7) + 0.25))      # any shift of the features, not only the mean
    assert abs(float(ref.cka_unbiased(shifted, raw_l) - ref.cka_unbiased(cen_k, cen_l))) < 1e-13


def test_cka_of_an_orthogonal_map_is_one():
    X = _features(4, 10, 6, 1.0).astype(np.float64)
    Q, _ = np.linalg.qr(np.random.RandomState(5).standard_normal((6, 6)))
    K, L = ref.gram(ref.centred(X, means=X.mean(0))), ref.gram((X @ Q).astype(LD) - (X @ Q).mean(0).astype(LD))
    assert abs(float(ref.cka_biased(K, L)) - 1.0) < 1e-13
    assert abs(float(ref.cka_unbiased(K, L)) - 1.0) < 1e-12


def test_independent_features_debiased_near_zero_biased_not():
    """n = 16 samples of 200 independent Gaussian features: the plain estimator sits near 0.93, the debiased one near 0"""
    b, u = [], []
    for seed in range(50):
        K, L = ref.centred_gram(_features(100 + seed, 16, 200)), ref.centred_gram(_features(200 + seed, 16, 200))
        b.append(float(ref.cka_biased(K, L)))
        u.append(float(ref.cka_unbiased(K, L)))
    assert np.mean(b) > 0.9
    assert abs(np.mean(u)) < 0.02


def test_means_are_the_contracts_fp64_sum_in_row_order():
    X = _features(6, 33, 5, 1e3)
    s = np.zeros(5)
    for i in range(33):
        s = s + X[i].astype(np.float64)
    assert np.array_equal(ref.column_means(X), s / 33.0)


def test_status_rules_and_the_nonpositive_self_term():
    X = _features(7, 6, 4)
    assert ref.status(X) == 0
    bad = X.copy()
    bad[2, 1] = np.inf
    assert ref.status(bad) == ref.NONFINITE
    assert ref.status(np.full((6, 4), 2.5, dtype=np.float32)) == ref.ZERO_VARIANCE
    Z, h = ref.nonpositive_self_layer()
    assert Z.shape == (4, 4) and h <= 0 and ref.status(Z) == ref.SELF_NOT_POSITIVE
    r = ref.scores([X[:4], Z], [Z, X[:4]])
    assert np.isnan(float(r["cka_unbiased"][0, 0])) and np.isfinite(float(r["cka"][0, 0]))
    assert np.isfinite(float(r["cka_unbiased"][0, 1])) and list(r["status_a"]) == [0, 4]


@pytest.mark.parametrize("name", sorted(cka_cases.CASES))
def test_cases_leave_the_bounds_no_room_to_excuse_a_wrong_kernel(name):
    """rho <= 100 for every layer, and every score at least 0.05 in magnitude unless the case is meant to be near zero:
    a tolerance of forward_bound is then below 1e-9 of any score it is applied to"""
    c = cka_cases.case(name)
    for K in c["ref"]["grams_a"] + c["ref"]["grams_b"]:
        assert 0 < ref.rho(K) <= 100
        assert 1 <= ref.kappa(K) <= np.sqrt(c["n"]) + 1e-9
    assert not c["ref"]["status_a"].any() and not c["ref"]["status_b"].any()
    cka, unb = np.array(c["ref"]["cka"], dtype=np.float64), np.array(c["ref"]["cka_unbiased"], dtype=np.float64)
    assert (np.abs(cka) >= 0.05).all()
    if name in cka_cases.NEAR_ZERO:
        assert (np.abs(unb) < 0.1).all() and (cka > 0.5).all()
    else:
        assert (np.abs(unb) >= 0.05).all()
    assert c["bound"][0].max() < 1e-10 and c["bound"][1].max() < 1e-9
    if name == "slabs":
        widths = sorted(X.shape[1] for X in c["a"] + c["b"])
        assert widths[-1] == 2 * ref.SLAB + 5 and {ref.SLAB - 1, ref.SLAB, ref.SLAB + 1} <= set(widths)
    assert ref.SLAB == engine.CKA_SLAB


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
    assert names == sorted(_hip.CKA_SIGNATURES)
    assert names == ["dt_cka", "dt_cka_gram", "dt_cka_min_workspace_bytes", "dt_cka_scores", "dt_cka_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    assert _hip.load(lib_path).dt_abi_version() == _hip.ABI_VERSION == 6
    for name, value in (("DT_CKA_MIN_N", engine.CKA_MIN_N), ("DT_CKA_MAX_N", engine.CKA_MAX_N), ("DT_CKA_SLAB", engine.CKA_SLAB),
                        ("DT_CKA_MAX_LAYERS", engine.CKA_MAX_LAYERS), ("DT_CKA_MAX_P", engine.CKA_MAX_P),
                        ("DT_CKA_SUM_ROWS", engine.CKA_SUM_ROWS)):
        assert header_constant(name) == value, name
    assert engine.CKA_SUMS == engine.CKA_SUM_ROWS + engine.CKA_MAX_N


def test_workspace_queries(lib_path):
    lib = _hip.load(lib_path)
    for n in (4, 64, 65, 2048):
        last = (0, 0)
        for p in (1, 3, 1024, 1025, 32768, 1 << 20, 1 << 24):
            least, full = lib.dt_cka_min_workspace_bytes(n, p), lib.dt_cka_workspace_bytes(8, n, p)
            tiles = ((n + 63) // 64) * ((n + 63) // 64 + 1) // 2
            assert least >= 8 * p + tiles * 4096 * 8 and full >= least > 0
            assert lib.dt_cka_workspace_bytes(1, n, p) == full == lib.dt_cka_workspace_bytes(64, n, p)   # layers take turns
            assert least >= last[0] and full >= last[1]                                                     # monotone in p
            last = (least, full)
    assert lib.dt_cka_min_workspace_bytes(64, 1024) < lib.dt_cka_min_workspace_bytes(65, 1024)
    for L, n, p in ((0, 8, 8), (65, 8, 8), (1, 3, 8), (1, 2049, 8), (1, 8, 0), (1, 8, (1 << 24) + 1), (1, -1, 8)):
        assert lib.dt_cka_workspace_bytes(L, n, p) == 0
    for n, p in ((3, 8), (2049, 8), (8, 0), (8, (1 << 24) + 1)):
        assert lib.dt_cka_min_workspace_bytes(n, p) == 0


def test_argument_paths_are_clean_under_asan_and_ubsan():
    """tests/host_sanitize/cka_driver.cpp: a program of its own, host code instrumented; it needs no GPU"""
    from distillation_trajectories_amd.csrc.build import build_cka_sanitizer_driver
    exe = build_cka_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "cka host checks clean" in res.stdout, res.stdout + res.stderr


def test_engine_checks_arguments_first_and_refuses_cpu_tensors(lib_path):
    _hip.load(lib_path)
    X = torch.zeros(6, 10)
    for bad in ([], [X] * 65, [torch.zeros(3, 10)], [torch.zeros(2049, 1)], [X.double()], [X.numpy()], [torch.zeros(6)],
                [X, torch.zeros(7, 10)], [torch.zeros(6, 0)], 5):
        with pytest.raises(ValueError):
            engine.device_cka_gram(bad)
        with pytest.raises(ValueError):
            engine.device_cka(bad)
        with pytest.raises(ValueError):
            engine.device_cka([X], bad)
    with pytest.raises(ValueError):
        engine.device_cka([X], [torch.zeros(7, 10)])
    for kw in (dict(workspace_bytes=-1), dict(workspace_bytes=1.5), dict(workspace_bytes=64)):
        with pytest.raises(ValueError):
            engine.device_cka_gram([X], **kw)
    view = torch.zeros(6, 2, 2, 8)
    for args in ((view, 0), (view, 9), (view, True), (view.double(), 4), (view[..., ::2], 2), (view[:, :, ::2], 4), (view[0], 4)):
        with pytest.raises(ValueError):
            engine.PitchedFeatures(*args)
    grams = engine.CkaGrams(torch.zeros(2, 6, 6, dtype=torch.float64), torch.zeros(2, engine.CKA_SUMS, dtype=torch.float64),
                            torch.zeros(2, dtype=torch.int32), 6)
    with pytest.raises(ValueError):
        engine.device_cka(grams._replace(n=5))
    with pytest.raises(ValueError):
        engine.device_cka(grams._replace(sums=torch.zeros(2, 8, dtype=torch.float64)))
    with pytest.raises(ValueError):
        engine.device_cka(grams, [torch.zeros(7, 3)])
    for call in (lambda: engine.device_cka_gram([X]), lambda: engine.device_cka([X]), lambda: engine.device_cka(grams),
                 lambda: engine.device_cka([engine.PitchedFeatures(view, 5)], [X])):
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            call()


def test_layers_are_described_in_place():
    """dense tensors keep their row stride, trailing axes are flattened; pitched views give groups, c and pitch"""
    buf = torch.zeros(6, 40)
    descs, n = engine._cka_layers([buf[:, 3:20], torch.zeros(6, 2, 3, 4), engine.PitchedFeatures(torch.zeros(7, 2, 3, 8)[1:], 5)], "a")
    assert n == 6
    assert descs[0][0].data_ptr() == buf.data_ptr() + 12 and descs[0][1:] == (40, 1, 17, 17)
    assert descs[1][1:] == (24, 1, 24, 24)
    assert descs[2][1:] == (48, 6, 5, 8)
    col = torch.zeros(10, 6).t()                       # no unit stride along the features: copied
    descs, _ = engine._cka_layers([col], "a")
    assert descs[0][1:] == (10, 1, 10, 10)
    p = engine.PitchedFeatures(torch.arange(4 * 1 * 2 * 4, dtype=torch.float32).view(4, 1, 2, 4), 3)
    assert p.n == 4 and p.dense()[1].tolist() == [8.0, 9.0, 10.0, 12.0, 13.0, 14.0]


def test_sweep_refuses_bad_sample_counts_and_resolutions_before_sampling(models):
    from distillation_trajectories_amd.config import Config
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 4
    teacher, student = models(0.1), models(0.05)
    for bad in (3, 2049, 0, 4.0, True):
        with pytest.raises(ValueError):
            representation.cka_sweep(teacher, [student], cfg, bad)
    with pytest.raises(ValueError):
        representation.cka_sweep(teacher, [], cfg, 8)
    with pytest.raises(ValueError):
        representation.cka_sweep(teacher, [student], cfg, 8, every=0)
    other = type("Other", (), {"image_size": 32})()
    with pytest.raises(ValueError, match="resolution"):
        representation.cka_sweep(teacher, [student, other], cfg, 8)
    with pytest.raises(ValueError):
        representation.cka_layers(teacher, student, torch.zeros(3, 3, 16, 16), torch.tensor([1]))
    assert metrics.cka_layers is representation.cka_layers and metrics.cka_sweep is representation.cka_sweep
    assert representation.BLOCKS == ("enc1", "enc2", "enc3", "enc4", "bottleneck", "dec3", "dec2", "dec1")
