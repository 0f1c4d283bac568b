"""The device t-SNE without a GPU: the float64 yardstick tsne_ref64 against sklearn's exact method (affinities, objective
and gradient, and the final KL of a full run within the chaos margin of tests/tsne_cases.py), the exported surface of
include/dt_hip_tsne.h, argument checks that fail before any device call, and the compiler's resource report of
csrc/dt_tsne.hip."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tsne_cases as cases
import tsne_ref64 as ref
from distillation_trajectories_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = [(12, 12), (102, 768), (130, 48)]


@pytest.mark.parametrize("shape", PINNED, ids=lambda s: f"n{s[0]}")
def test_affinities_match_sklearn_joint_probabilities(shape):
    """within 2e-7 of max P: sklearn takes the squared distances in float32 (8e-8 was measured)"""
    t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    from sklearn.metrics import pairwise_distances
    c = cases.case(*shape)
    D = pairwise_distances(c["X"], metric="euclidean", squared=True)
    want = squareform(t_sne._joint_probabilities(D, c["perplexity"], 0))
    gap = np.abs(c["P"] - want).max() / c["P"].max()
    print(shape, "affinity gap / max P", gap)
    assert gap <= 2e-7
    assert np.array_equal(c["P"], c["P"].T) and np.all(np.diag(c["P"]) == 0.0)
    assert abs(c["P"].sum() - 1.0) < 1e-12


@pytest.mark.parametrize("shape", PINNED, ids=lambda s: f"n{s[0]}")
def test_objective_and_gradient_match_sklearn(shape):
    t_sne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    c = cases.case(*shape)
    n = shape[0]
    for seed, scale in ((1, 1.0), (2, 1e-4), (3, 30.0)):
        Y = scale * np.random.RandomState(seed).standard_normal((n, 2))
        kl, grad = ref.kl_grad(Y, c["P"])
        kl_sk, grad_sk = t_sne._kl_divergence(Y.ravel(), squareform(c["P"], checks=False), 1, n, 2)
        assert abs(kl - kl_sk) <= 1e-12 * abs(kl_sk), (shape, seed)
        assert np.abs(grad.ravel() - grad_sk).max() <= 1e-12 * np.abs(grad_sk).max(), (shape, seed)


@pytest.mark.parametrize("shape", [(102, 768), (130, 48)], ids=lambda s: f"n{s[0]}")
def test_full_run_kl_agrees_with_sklearn_within_the_chaos_margin(shape):
    """1000 iterations from the same Y0: the embeddings differ by a good part of their extent (the optimiser is chaotic),
    the KL by no more than 3 s of tsne_cases.CHAOS_SPREAD."""
    TSNE = pytest.importorskip("sklearn.manifold").TSNE
    c = cases.case(*shape)
    assert c["final"]["n_iter"] == 1000 and c["final"]["stop"] == ref.RUNNING
    kl_ref = ref.final_kl(c["final"], c["P"])
    sk = TSNE(method="exact", init=c["Y0"], perplexity=c["perplexity"], max_iter=1000).fit(c["X"])
    rel = abs(sk.kl_divergence_ - kl_ref) / kl_ref
    print(shape, "KL yardstick", kl_ref, "sklearn", sk.kl_divergence_, "relative", rel)
    assert rel <= cases.CHAOS_FACTOR * cases.CHAOS_SPREAD[shape]


def test_stage_reset_and_stop_rules_of_the_yardstick():
    c = cases.case(65, 48)
    s = c["states"][250]
    assert np.any(s["update"] != 0.0) and s["n_iter"] == 250          # the state before iteration 250 is not yet reset
    after = ref.descend(s, c["P"], 250, 251, c["params"])
    fresh = dict(ref.copy_state(s), update=np.zeros_like(s["y"]), gains=np.ones_like(s["y"]))
    again = ref.descend(fresh, c["P"], 250, 251, c["params"])
    assert np.array_equal(after["y"], again["y"]) and after["best_iter"] == 250
    stuck = dict(ref.copy_state(c["states"][300]), best_error=0.0, best_iter=-1)
    out = ref.descend(stuck, c["P"], 300, 1000, c["params"])
    assert out["n_iter"] == 350 and out["stop"] == ref.NO_PROGRESS
    quick = ref.descend(ref.new_state(c["Y0"]), c["P"], 0, 1000, dict(c["params"], min_grad_norm=1e300))
    assert quick["n_iter"] == 50 and quick["stop"] == ref.GRAD_NORM
    assert c["tie_margin"] >= 1e-9


def _tsne_header_functions():
    text = open(os.path.join(ROOT, "include", "dt_hip_tsne.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#define[^\n]*", "", text)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_exports_agree():
    from distillation_trajectories_amd.csrc.build import HEADERS, LIB, SOURCES, build
    assert "dt_tsne.hip" in SOURCES and any(h.endswith("dt_hip_tsne.h") for h in HEADERS)
    path = build() if not os.path.exists(LIB) else LIB
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    names = _tsne_header_functions()
    assert names == ["dt_tsne_affinities", "dt_tsne_descend", "dt_tsne_workspace_bytes"]
    assert sorted(_hip.TSNE_SIGNATURES) == names
    assert set(names) <= exported
    others = (set(_hip.SIGNATURES) | set(_hip.NOISE_SIGNATURES) | set(_hip.INCEPTION_SIGNATURES) | set(_hip.PCA_SIGNATURES)
              | set(_hip.FID_SIGNATURES) | set(_hip.LPIPS_SIGNATURES))
    assert not set(names) & others
    lib = _hip.load(path)
    assert lib.dt_abi_version() == _hip.ABI_VERSION == 6
    assert all(getattr(lib, n).argtypes is not None for n in names)
    # dt_tsne_params as the header lays it out: 6 doubles, then 4 ints
    assert ctypes.sizeof(_hip.TsneParams) == 6 * 8 + 4 * 4
    assert [f[0] for f in _hip.TsneParams._fields_] == re.findall(
        r"^  (?:double|int) (\w+)", open(os.path.join(ROOT, "include", "dt_hip_tsne.h")).read(), flags=re.M)


def test_workspace_query_rejects_shapes_outside_the_limits():
    lib = _hip.load()
    assert lib.dt_tsne_workspace_bytes(256, 202, 3072) > 256 * 2 * 202 * 202 * 8
    assert lib.dt_tsne_workspace_bytes(1, 4, 4) > 0 and lib.dt_tsne_workspace_bytes(65535, 512, 4) > 0
    for args in ((0, 10, 8), (65536, 10, 8), (1, 3, 8), (1, 513, 8), (1, 10, 6), (1, 10, 0), (1, 10, -4)):
        assert lib.dt_tsne_workspace_bytes(*args) == 0, args


def test_entries_reject_bad_arguments_without_a_device():
    """every refusal comes back before the first HIP call: the pointers are never dereferenced"""
    lib = _hip.load()
    a = ctypes.c_void_p(4096)                     # 16-byte aligned, never read
    odd = ctypes.c_void_p(4100)

    def aff(a_ptr=a, n_a=6, a_ps=8, a_rs=16, b_ptr=a, n_b=6, b_ps=8, b_rs=16, P=2, E=8, perp=3.0, p=a, st=a, ws=a, nb=1 << 30):
        return lib.dt_tsne_affinities(a_ptr, n_a, a_ps, a_rs, b_ptr, n_b, b_ps, b_rs, P, E, perp, p, st, ws, nb, None)
    null, shape, arg, small = -1, -2, -3, -4
    assert aff(a_ptr=None) == null and aff(b_ptr=None) == null and aff(p=None) == null and aff(st=None) == null
    assert aff(ws=None) == null
    for kw in (dict(n_a=0), dict(n_b=-1), dict(n_a=2, n_b=1), dict(n_a=512, n_b=1), dict(P=0), dict(P=65536), dict(E=6),
               dict(E=0)):
        assert aff(**kw) == shape, kw
    for kw in (dict(perp=0.0), dict(perp=12.0), dict(perp=-1.0), dict(perp=float("nan")), dict(a_ptr=odd), dict(a_rs=18),
               dict(b_ps=6), dict(ws=odd)):
        assert aff(**kw) == arg, kw
    assert aff(nb=64) == small

    def prm(**over):
        p = _hip.TsneParams(12.0, 200.0, (ctypes.c_double * 2)(0.5, 0.8), 0.01, 1e-7, 250, 50, (ctypes.c_int * 2)(250, 300))
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def desc(p=a, P=2, n=10, st=a, b=0, e=10, params=prm(), emb=a, kl=a):
        return lib.dt_tsne_descend(p, P, n, st, b, e, ctypes.byref(params) if params is not None else None, emb, kl, None)
    assert desc(p=None) == null and desc(st=None) == null and desc(params=None) == null and desc(emb=None) == null
    assert desc(kl=None) == null
    for kw in (dict(P=0), dict(P=65536), dict(n=3), dict(n=513)):
        assert desc(**kw) == shape, kw
    for kw in (dict(b=-1), dict(b=11), dict(params=prm(n_iter_check=0)), dict(params=prm(exaggeration_iters=-1)),
               dict(params=prm(learning_rate=0.0)), dict(params=prm(early_exaggeration=float("nan"))),
               dict(params=prm(min_gain=-1.0)), dict(params=prm(min_grad_norm=-1.0))):
        assert desc(**kw) == arg, kw


def test_bad_arguments_raise_before_any_device_call(monkeypatch):
    from distillation_trajectories_amd import engine
    from distillation_trajectories_amd.analysis.dimensionality.tsne import TrajectoryTSNE

    def no_load(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_hip, "load", no_load)
    a, y0 = torch.zeros(5, 3, 8), torch.zeros(5, 2)
    with pytest.raises(ValueError, match="4 <= n <= 512"):
        engine.device_tsne(torch.zeros(3, 3, 8), perplexity=1.0, init=torch.zeros(3, 2))
    with pytest.raises(ValueError, match="4 <= n <= 512"):
        engine.device_tsne(torch.zeros(300, 1, 8), torch.zeros(213, 1, 8), perplexity=1.0, init=torch.zeros(513, 2))
    with pytest.raises(ValueError, match="does not match"):
        engine.device_tsne(a, torch.zeros(4, 3, 12), perplexity=2.0, init=torch.zeros(9, 2))
    with pytest.raises(ValueError, match="float32"):
        engine.device_tsne(a.double(), perplexity=2.0, init=y0)
    for perp in (0, -1.0, 5, 5.5, float("nan"), "30", None, True):
        with pytest.raises(ValueError, match="perplexity"):
            engine.device_tsne(a, perplexity=perp, init=y0)
    with pytest.raises(ValueError, match="exactly one of init"):
        engine.device_tsne(a, perplexity=2.0)
    with pytest.raises(ValueError, match="exactly one of init"):
        engine.device_tsne(a, perplexity=2.0, init=y0, state=torch.zeros(3, 34, dtype=torch.float64))
    with pytest.raises(ValueError, match="init must be"):
        engine.device_tsne(a, perplexity=2.0, init=torch.zeros(5, 3))
    with pytest.raises(ValueError, match="init must be"):
        engine.device_tsne(a, perplexity=2.0, init=torch.zeros(2, 5, 2))
    with pytest.raises(ValueError, match="state must be"):
        engine.device_tsne(a, perplexity=2.0, state=torch.zeros(3, 33, dtype=torch.float64))
    with pytest.raises(ValueError, match="state must be"):
        engine.device_tsne(a, perplexity=2.0, state=torch.zeros(3, 34))
    with pytest.raises(ValueError, match="affinities must be"):
        engine.device_tsne(a, perplexity=2.0, init=y0, affinities=torch.zeros(3, 5, 4, dtype=torch.float64))
    for kw, what in ((dict(max_iter=-1), "max_iter"), (dict(max_iter=2.5), "max_iter"), (dict(it_begin=7, max_iter=5), "max_iter"),
                     (dict(it_begin=-1), "it_begin"), (dict(learning_rate="fast"), "learning_rate"),
                     (dict(learning_rate=0.0), "learning_rate"), (dict(early_exaggeration=0.0), "early_exaggeration"),
                     (dict(min_grad_norm=-1.0), "min_grad_norm"), (dict(n_iter_without_progress=-1), "n_iter_without_progress"),
                     (dict(n_iter_check=0), "n_iter_check"), (dict(momentum=0.5), "momentum"), (dict(min_gain=-0.1), "min_gain"),
                     (dict(exaggeration_iters=-5), "exaggeration_iters")):
        with pytest.raises(ValueError, match=what):
            engine.device_tsne(a, perplexity=2.0, init=y0, **kw)

    X = np.zeros((12, 8), np.float32)
    for kw in (dict(n_components=3), dict(n_components=1), dict(init="spectral"), dict(init=np.zeros((11, 2))),
               dict(perplexity=12.0), dict(perplexity=0), dict(learning_rate="slow"), dict(max_iter=-3),
               dict(early_exaggeration=-1.0), dict(min_grad_norm=-1e-7), dict(n_iter_without_progress=2.5)):
        with pytest.raises(ValueError):
            TrajectoryTSNE(**kw).fit(X)
    with pytest.raises(ValueError):
        TrajectoryTSNE(perplexity=0.5).fit(np.zeros((3, 8), np.float32))          # fewer than 4 rows
    with pytest.raises(ValueError):
        TrajectoryTSNE().fit([[0.0] * 8] * 12)                                     # neither an array nor a tensor
    doc = TrajectoryTSNE.__doc__
    assert 'method="exact"' in doc and "barnes_hut" in doc


def test_tsne_kernels_do_not_spill():
    """every kernel of csrc/dt_tsne.hip, the shared csrc/dt_dense64.h kernels included: tools/kernel_resources.py compiles
    the file device-only for gfx950 and reads the compiler's own resource remarks (nothing is run)"""
    from distillation_trajectories_amd.csrc.build import hipcc_path
    try:
        hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc is not installed")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    res = tool.kernel_resources("dt_tsne.hip")
    own = {"tsne_mean_kernel", "tsne_gram_kernel", "tsne_row_kernel", "tsne_joint_kernel", "tsne_descend_kernel"}
    assert own <= set(res), sorted(res)
    for name, r in sorted(res.items()):
        print(f"dt_tsne.hip {name}: {r['vgprs']} VGPRs, {r['vgpr_spill']} spilled, {r['scratch_bytes']} B scratch")
    bad = {n: (r["vgpr_spill"], r["scratch_bytes"]) for n, r in res.items() if r["vgpr_spill"] or r["scratch_bytes"]}
    assert not bad, f"(spilled VGPRs, scratch bytes per lane): {bad}"
