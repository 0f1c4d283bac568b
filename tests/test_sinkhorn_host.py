"""Sinkhorn divergence without a GPU: the yardstick sinkhorn_ref64 against facts that do not depend on it (the exact
assignment cost from scipy, symmetry, closed forms), its bound, the derived Python quantities, the exported surface of
include/dt_hip_sinkhorn.h, the size query, the sanitizer driver, the compiler's resource report, and argument checks that
fail before any device call."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import sinkhorn_ref64 as ref
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.analysis import metrics
from distillation_trajectories_amd.analysis.metrics import sinkhorn as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dt_hip_sinkhorn.h")
GAUSS = [(64, 64, 48), (64, 64, 2)]


def gauss_case(n_a, n_b, E, p=2, rel=0.05):
    a, b = ref.sets(2, 1, n_a, n_b, E)
    a, b = a[0], b[0]
    return a, b, ref.cost(a, b, p), ref.epsilon(a, b, p, rel)


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("p", [1, 2])
def test_single_rows_give_the_cost(p):
    a, b = np.float32([[1.5, -2.0, 0.25]]), np.float32([[0.5, 1.0, 4.0]])
    C = ref.cost(a, b, p)
    want = 1.0 + 9.0 + 3.75 ** 2
    assert float(C[0, 0]) == (want if p == 2 else float(np.sqrt(ref.LD(want))))
    for eps in (0.01, 1.0, 100.0):
        r = ref.iterate(C, eps, 3)
        assert abs(r["ot"] - C[0, 0]) <= 4 * 2.0 ** -64 * C[0, 0] and r["err"] == 0 and r["iters"] == 3
        assert ref.iterate(C, eps, 9, tol=1e-12)["iters"] == 1


@pytest.mark.parametrize("n_a,n_b,E", GAUSS)
def test_entropic_cost_brackets_the_assignment_cost(n_a, n_b, E):
    """W <= OT_eps <= W + eps log n for equal sizes and uniform weights, W the exact assignment cost"""
    a, b, C, eps = gauss_case(n_a, n_b, E)
    r = ref.iterate(C, eps, 5000, tol=1e-10)
    assert r["status"] == 0 and r["err"] <= 1e-10
    C64 = C.astype(np.float64)
    rows, cols = linear_sum_assignment(C64)
    W = C64[rows, cols].mean()
    slack = 1e-8 * W                                    # the dual value of a plan whose marginals are within 1e-10
    print(f"({n_a},{n_b},{E}): W={W:.6f} ot={float(r['ot']):.6f} W+eps log n={W + eps * np.log(n_a):.6f} steps={r['iters']}")
    assert W - slack <= r["ot"] <= W + eps * np.log(n_a) + slack
    assert r["ot"] - W > 1e-3 * eps and W + eps * np.log(n_a) - r["ot"] > 1e-3 * eps          # strictly inside


@pytest.mark.parametrize("n_a,n_b,E", GAUSS + [(37, 64, 19)])
def test_symmetry_and_update_order_at_convergence(n_a, n_b, E):
    a, b, C, eps = gauss_case(n_a, n_b, E)
    r = ref.iterate(C, eps, 5000, tol=1e-12)
    swapped = ref.iterate(ref.cost(b, a, 2), eps, 5000, tol=1e-12)
    assert abs(r["ot"] - swapped["ot"]) <= 1e-9 * abs(r["ot"])
    Caa = ref.cost(a, a, 2)
    assert (np.diag(Caa) == 0).all() and (Caa >= 0).all() and (Caa == Caa.T).all()
    first, second = ref.iterate(Caa, eps, 5000, tol=1e-12), ref.iterate(Caa, eps, 5000, tol=1e-12, f_first=False)
    assert abs(first["ot"] - second["ot"]) <= 1e-9 * abs(first["ot"])
    div = ref.divergence(r["ot"], first["ot"], ref.iterate(ref.cost(b, b, 2), eps, 5000, tol=1e-12)["ot"])
    assert div > 0


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("n_a,n_b,E,K", [(64, 64, 48, 50), (37, 64, 19, 50), (5, 3, 1, 50), (64, 64, 2, 400)])
def test_plain_float64_stays_within_the_forward_bound(n_a, n_b, E, K, p):
    a, b, C, eps = gauss_case(n_a, n_b, E, p)
    want = ref.iterate(C, eps, K)
    bound = ref.forward_bound(C, eps, want, E, p)
    C64 = ref.cost(a, b, p, np.float64)
    got = ref.iterate(C64, eps, K)
    assert (np.abs(C64 - C) <= ref.cost_bound(C, E, p)).all()
    assert abs(float(C64.mean()) - C.mean()) <= ref.mean_cost_bound(C, E, p)
    for key in ("ot", "err", "f", "g"):
        err = np.abs(np.asarray(got[key]).astype(ref.LD) - want[key]).max()
        print(f"({n_a},{n_b},{E}) p={p} {key}: |float64 - extended| = {float(err):.3g}, bound {bound[key]:.3g}")
        assert err <= bound[key], key
    assert got["iters"] == want["iters"] == K and got["status"] == want["status"] == 0
    assert 0 < ref.divergence_bound(bound["ot"], bound["ot"], bound["ot"], want["ot"]) < 3 * bound["ot"]


def test_the_bound_is_a_tolerance_not_a_loophole():
    """(64, 64, 48), p = 2, rel_epsilon 0.05, 50 steps: the cost term alone is 2 K (E + 1) u max c, near 1e-10, so the bound
    on ot cannot be below that; it has to stay within a few times it, twelve digits of the value"""
    a, b, C, eps = gauss_case(64, 64, 48)
    r = ref.iterate(C, eps, 50)
    bound = ref.forward_bound(C, eps, r, 48, 2)
    floor = 2 * 50 * 49 * ref.U * float(C.max())
    print(f"ot={float(r['ot']):.6f} eps={eps:.6f} bound: " + " ".join(f"{k}={v:.3g}" for k, v in bound.items()), f"cost term {floor:.3g}")
    assert 70 < r["ot"] < 90
    assert floor < bound["f"] < 1.5 * floor and 2 * floor < bound["ot"] < 3 * floor < 1e-9
    assert bound["ot"] < 1e-11 * r["ot"]
    assert ref.status(np.zeros((3, 2, 2)), np.zeros((2, 2)), [1.0, 0.0, np.inf]).tolist() == [0, 2, 2]
    bad = np.zeros((3, 2, 2))
    bad[1, 0, 1] = np.nan
    assert ref.status(bad, np.zeros((3, 4, 2)), [1.0, -1.0, 2.0]).tolist() == [0, 3, 0]


def test_stopping_rule_of_the_yardstick():
    a, b, C, eps = gauss_case(37, 64, 19)
    free = ref.iterate(C, eps, 300)
    k = next(i for i, e in enumerate(free["errs"], 1) if e <= 1e-8)
    stopped = ref.iterate(C, eps, 300, tol=1e-8)
    assert stopped["iters"] == k and stopped["status"] == 0 and stopped["err"] == free["errs"][k - 1]
    assert stopped["ot"] == ref.iterate(C, eps, k)["ot"]
    short = ref.iterate(C, eps, k - 1, tol=1e-8)
    assert short["iters"] == k - 1 and short["status"] == ref.NOT_CONVERGED


# ------------------------------------------------------------------------------------------------ derived quantities
def test_relative_epsilon_and_exports():
    assert sk.relative_epsilon(np.array([2.0, 0.0, np.nan]), 0.25)[:2].tolist() == [0.5, 0.0]
    t = sk.relative_epsilon(torch.tensor([2.0, 8.0], dtype=torch.float64), 0.05)
    assert t.dtype == torch.float64 and t.tolist() == [2.0 * 0.05, 8.0 * 0.05]
    for bad in (0, -0.1, np.inf, np.nan, True, None, "0.05"):
        with pytest.raises(ValueError):
            sk.relative_epsilon(1.0, bad)
    assert sk.teacher_epsilon(None, 0.75, 0.05, 2) == 0.75                      # a given epsilon is taken as it is
    assert metrics.sinkhorn_pairs is sk.sinkhorn_pairs and metrics.sinkhorn_trajectories is sk.sinkhorn_trajectories
    assert metrics.sinkhorn_sweep is sk.sinkhorn_sweep
    assert sk.DEFAULT_REL_EPSILON == 0.05 and 1 <= engine.SINKHORN_DEFAULT_MAX_ITER <= engine.SINKHORN_MAX_ITER
    assert engine.SINKHORN_DEFAULT_TOL > 0


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
    assert names == sorted(_hip.SINKHORN_SIGNATURES)
    assert names == ["dt_sinkhorn_mean_cost", "dt_sinkhorn_ot", "dt_sinkhorn_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    assert _hip.load(lib_path).dt_abi_version() == _hip.ABI_VERSION == 6
    for name, value in (("DT_SINKHORN_MAX_N", engine.SINKHORN_MAX_N), ("DT_SINKHORN_MAX_E", engine.SINKHORN_MAX_E),
                        ("DT_SINKHORN_MAX_P", engine.SINKHORN_MAX_P), ("DT_SINKHORN_MAX_ITER", engine.SINKHORN_MAX_ITER),
                        ("DT_SINKHORN_OK", engine.SINKHORN_OK), ("DT_SINKHORN_NONFINITE", engine.SINKHORN_NONFINITE),
                        ("DT_SINKHORN_BAD_EPS", engine.SINKHORN_BAD_EPS),
                        ("DT_SINKHORN_NOT_CONVERGED", engine.SINKHORN_NOT_CONVERGED)):
        assert header_constant(name) == value, name
    assert (ref.NONFINITE, ref.BAD_EPS, ref.NOT_CONVERGED) == (1, 2, 4)
    assert "dt_sinkhorn" not in open(os.path.join(ROOT, "include", "dt_hip.h")).read()       # nothing is added to dt_hip.h
    lib = _hip.load(lib_path)
    names = set()
    for cls in range(lib.dt_profile_class_count()):
        name = _hip.c_char_p()
        n, ms, fl, by = _hip.c_longlong(), _hip.c_double(), _hip.c_double(), _hip.c_double()
        assert lib.dt_profile_read(cls, name, n, ms, fl, by) == 0
        names.add(name.value.decode())
    assert {"sinkhorn_scan_kernel", "sinkhorn_init_kernel", "sinkhorn_cost_kernel", "sinkhorn_row_kernel", "sinkhorn_col_kernel",
            "sinkhorn_finish_kernel", "sinkhorn_rowsum_kernel", "sinkhorn_mean_kernel"} <= names       # a class per kernel


def test_size_query(lib_path):
    lib = _hip.load(lib_path)
    for P, n_a, n_b in ((1, 1, 1), (3, 7, 65), (51, 256, 256), (1 << 16, 2048, 2048), (5, 2048, 3)):
        one, many = lib.dt_sinkhorn_workspace_bytes(1, n_a, n_b), lib.dt_sinkhorn_workspace_bytes(P, n_a, n_b)
        assert one >= 8 * (n_a * n_b + n_a + 2 * n_b) and one % 8 == 0 and many == P * one
        if P > 1:
            assert lib.dt_sinkhorn_workspace_bytes(P - 1, n_a, n_b) < many                  # monotone in P
    for P, n in ((0, 4), (65537, 4), (1, 0), (1, 2049), (-1, 4), (1, -3)):
        assert lib.dt_sinkhorn_workspace_bytes(P, n, 4) == 0 and lib.dt_sinkhorn_workspace_bytes(P, 4, n) == 0


def test_argument_paths_are_clean_under_asan_and_ubsan():
    """tests/host_sanitize/sinkhorn_driver.cpp: a program of its own, host code instrumented; it needs no GPU"""
    from distillation_trajectories_amd.csrc.build import build_sinkhorn_sanitizer_driver
    exe = build_sinkhorn_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "sinkhorn host checks clean" in res.stdout, res.stdout + res.stderr


def test_no_kernel_spills_or_uses_scratch():
    """every kernel of csrc/dt_sinkhorn.hip: tools/kernel_resources.py compiles the file device-only for gfx950 and reads the
    compiler's own resource remarks (nothing is run)"""
    from distillation_trajectories_amd.csrc.build import hipcc_path
    try:
        hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc is not installed")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    res = tool.kernel_resources("dt_sinkhorn.hip")
    own = {"sinkhorn_scan_kernel", "sinkhorn_init_kernel", "sinkhorn_cost_kernel", "sinkhorn_rowsum_kernel", "sinkhorn_mean_kernel",
           "sinkhorn_row_kernel", "sinkhorn_col_kernel", "sinkhorn_finish_kernel"}
    assert own == {n for n in res if n.startswith("sinkhorn_")}, sorted(res)
    for name, r in sorted(res.items()):
        print(f"dt_sinkhorn.hip {name}: {r['vgprs']} VGPRs, {r['vgpr_spill']} spilled, {r['scratch_bytes']} B scratch, {r['lds_bytes']} B LDS")
    bad = {n: (r["vgpr_spill"], r["sgpr_spill"], r["scratch_bytes"]) for n, r in res.items()
           if r["vgpr_spill"] or r["sgpr_spill"] or r["scratch_bytes"]}
    assert not bad, f"(spilled VGPRs, spilled SGPRs, scratch bytes per lane): {bad}"
    assert all(res[n]["lds_bytes"] <= 64 * 1024 for n in own)


def test_engine_checks_arguments_first(lib_path):
    _hip.load(lib_path)
    X = torch.zeros(3, 4, 12)
    calls = (lambda a, b, **kw: engine.device_sinkhorn_ot(a, b, 1.0, **kw),
             lambda a, b, **kw: engine.device_sinkhorn_divergence(a, b, 1.0, **kw),
             lambda a, b, **kw: engine.device_sinkhorn_mean_cost(a, b, **{k: v for k, v in kw.items() if k in ("p", "workspace_bytes")}))
    for call in calls:
        for bad in (X.double(), X.half(), X.numpy(), None, torch.zeros(12), torch.zeros(2, 2, 2, 12), [X], torch.zeros(3, 0, 12),
                    torch.zeros(3, 2049, 2), torch.zeros(3, 4, 0)):                              # type, dtype, dims, limits
            with pytest.raises(ValueError):
                call(bad, X)
            with pytest.raises(ValueError):
                call(X, bad)
        with pytest.raises(ValueError):
            call(X, torch.zeros(3, 4, 13))                                                       # another width
        with pytest.raises(ValueError):
            call(X, torch.zeros(2, 4, 12))                                                       # 3 states against 2
        for p in (0, 3, 2.0, True, None):
            with pytest.raises(ValueError):
                call(X, X, p=p)
        for ws in (-1, 1.5, True):
            with pytest.raises(ValueError):
                call(X, X, workspace_bytes=ws)
        with pytest.raises(ValueError, match="on the device"):                                   # wrong device, last
            call(X, X)
        with pytest.raises(ValueError, match="on the device"):
            call(X, X[0], p=1)
    for call in calls[:2]:
        for it in (0, -1, 10001, 2.0, True):
            with pytest.raises(ValueError):
                call(X, X, max_iter=it)
        for tol in (-1e-9, np.inf, np.nan, True, None, "1e-9"):
            with pytest.raises(ValueError):
                call(X, X, tol=tol)
    for fn in (engine.device_sinkhorn_ot, engine.device_sinkhorn_divergence):
        for eps in (0.0, -1.0, np.inf, np.nan, True, None, "1", torch.ones(3), torch.ones(2, dtype=torch.float64),
                    torch.ones(3, 1, dtype=torch.float64)):
            with pytest.raises(ValueError):
                fn(X, X, eps)
        with pytest.raises(ValueError, match="on the device"):
            fn(X, X, torch.ones(3, dtype=torch.float64))
    ot = torch.zeros(3, dtype=torch.float64)
    for bad in (ot.float(), torch.zeros(2, dtype=torch.float64), torch.zeros(3, 1, dtype=torch.float64), 1.0, {"ot": ot.float()}):
        with pytest.raises(ValueError, match="self_a"):
            engine.device_sinkhorn_divergence(X, X, 1.0, self_a=bad)
        with pytest.raises(ValueError, match="self_b"):
            engine.device_sinkhorn_divergence(X, X, 1.0, self_b=bad)
    with pytest.raises(ValueError, match="on the device"):
        engine.device_sinkhorn_divergence(X, X, 1.0, self_a=ot, self_b={"ot": ot})
    with pytest.raises(ValueError):
        sk.sinkhorn_pairs(X, X.double(), epsilon=1.0)
    with pytest.raises(ValueError):
        sk.sinkhorn_pairs(X, X, epsilon=1.0, rel_epsilon=0.0)
    with pytest.raises(ValueError, match="on the device"):
        sk.sinkhorn_pairs(X, X)


def test_trajectory_forms_and_sweep_arguments(models):
    from distillation_trajectories_amd.config import Config
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 4
    teacher, student = models(0.1), models(0.05)
    for bad in (0, 1, 3, -1, 4.0, True, 2049):
        with pytest.raises(ValueError):
            sk.sinkhorn_sweep(teacher, [student], cfg, [1.0], bad)
    with pytest.raises(ValueError):
        sk.sinkhorn_sweep(teacher, [], cfg, [1.0], 4)
    with pytest.raises(ValueError):
        sk.sinkhorn_sweep(teacher, [student], cfg, [], 4)
    with pytest.raises(ValueError):
        sk.sinkhorn_sweep(teacher, [student], cfg, [1.0], 4, every=0)
    for kw in (dict(p=3), dict(rel_epsilon=0.0), dict(epsilon=-1.0), dict(max_iter=0), dict(tol=-1.0)):
        with pytest.raises(ValueError):
            sk.sinkhorn_sweep(teacher, [student], cfg, [1.0], 4, **kw)
    other = type("Other", (), {"image_size": 32})()
    with pytest.raises(ValueError, match="resolution"):
        sk.sinkhorn_sweep(teacher, [student, other], cfg, [1.0], 4)
    a = [torch.zeros(2, 3, 4, 4) for _ in range(3)]
    with pytest.raises(ValueError, match="states"):
        sk.sinkhorn_trajectories(a, a[:2])                                    # unequal lengths are refused
