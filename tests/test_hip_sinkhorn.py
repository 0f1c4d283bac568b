"""GPU: the entropic transport cost and the Sinkhorn divergence (include/dt_hip_sinkhorn.h, engine.device_sinkhorn_*,
analysis/metrics/sinkhorn.py) against the extended-precision yardstick tests/sinkhorn_ref64.py within the bounds derived
there, the header's five bit contracts, the stopping rule, the status bits and the analysis layer.  Observed error over
bound on an MI355X: DESIGN §9ah."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import sinkhorn_ref64 as ref
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.analysis.metrics import sinkhorn as sk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOW = (64, 64, 2)                 # needs a few hundred steps: 400 are run, 50 everywhere else
SHAPES = [(1, 1, 1), (5, 3, 1), (3, 5, 7), (64, 64, 48), (65, 130, 17), (37, 64, 19), (2048, 3, 5), (3, 2048, 5), SLOW,
          (200, 200, 768)]
SMALL = [s for s in SHAPES if max(s[:2]) <= 130]
OUT = ("ot", "err", "iters", "status", "f", "g")
ids = lambda s: "x".join(map(str, s))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t) for t in (a, b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.int64), b.view(np.int64)) if a.dtype == np.float64 else np.array_equal(a, b)


def same_outputs(x, y, keys=OUT):
    return all(same_bits(x[k], y[k]) for k in keys)


def run(a, b, eps, p=2, max_iter=30, tol=0.0, **kw):
    return engine.device_sinkhorn_ot(a, b, eps, p=p, max_iter=max_iter, tol=tol, potentials=True, **kw)


def ratios(out, q, want, bound):
    """|device - yardstick| / bound of ot, err, f, g for problem q of a device result"""
    worst = {}
    for key in ("ot", "err", "f", "g"):
        err = float(np.abs(out[key][q].cpu().numpy().astype(ref.LD) - want[key]).max())
        assert bound[key] > 0
        worst[key] = err / bound[key]
    return worst


# ------------------------------------------------------------------------------------------------ tolerance
@functools.lru_cache(maxsize=None)
def inputs(shape):
    """a [n_a, E], b [3, n_b, E] and the three squared-distance matrices in extended precision"""
    n_a, n_b, E = shape
    a3, b = ref.sets(1000 * n_a + 10 * n_b + E, 3, n_a, n_b, E)
    return a3[0], b, [ref.cost(a3[0], b[q], 2) for q in range(3)]


@functools.lru_cache(maxsize=None)
def reference(shape, p, rel):
    """3 problems: set a [n_a, E] is shared by all of them (problem stride 0), b [3, n_b, E] differs from problem to
    problem, and so does epsilon (the middle one is half as large again).  Per problem the yardstick's run of K steps and
    its bounds, made once."""
    E, K = shape[2], 400 if shape == SLOW else 50
    a, b, squares = inputs(shape)
    eps = [ref.epsilon(a, b[q], p, rel) * (1.0, 1.5, 1.0)[q] for q in range(3)]
    runs = []
    for q in range(3):
        C = squares[q] if p == 2 else np.sqrt(squares[q])
        res = ref.iterate(C, eps[q], K)
        runs.append({"res": res, "bound": ref.forward_bound(C, eps[q], res, E, p), "mean_cost": C.mean(),
                     "mean_cost_bound": ref.mean_cost_bound(C, E, p)})
    return a, b, eps, K, runs


@pytest.mark.parametrize("rel", [0.05, 0.25])
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_outputs_within_the_forward_bound(shape, p, rel):
    a, b, eps, K, runs = reference(shape, p, rel)
    da, db = dev(a), dev(b)
    out = run(da, db, dev(np.float64(eps)), p, max_iter=K)
    mc = engine.device_sinkhorn_mean_cost(da, db, p=p)
    assert out["iters"].tolist() == [K] * 3 and out["status"].tolist() == [0] * 3 and mc["status"].tolist() == [0] * 3
    assert out["f"].shape == (3, shape[0]) and out["g"].shape == (3, shape[1])
    worst = dict.fromkeys(("ot", "err", "f", "g", "mean_cost"), 0.0)
    for q, r in enumerate(runs):
        got = ratios(out, q, r["res"], r["bound"])
        got["mean_cost"] = float(abs(ref.LD(mc["mean_cost"][q].item()) - r["mean_cost"])) / r["mean_cost_bound"]
        worst = {k: max(worst[k], got[k]) for k in worst}
    print(f"{ids(shape)} p={p} rel_epsilon={rel}: error / bound " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


# ------------------------------------------------------------------------------------------------ contracts
@pytest.fixture(scope="module", params=[(5, 3, 7), (65, 130, 17), (37, 64, 19)], ids=ids)
def batch(request):
    """3 problems on contiguous tensors, one epsilon each, and their outputs after 30 steps for both p: what every
    variation below has to reproduce"""
    n_a, n_b, E = request.param
    a, b = ref.sets(n_a + n_b + E, 3, n_a, n_b, E)
    made = {"shape": request.param, "a": dev(a), "b": dev(b)}
    for p in (1, 2):
        eps = dev(np.float64([ref.epsilon(a[q], b[q], p, 0.25) * (1.0, 0.5, 2.0)[q] for q in range(3)]))
        made[p] = {"eps": eps, "want": run(made["a"], made["b"], eps, p)}
        assert made[p]["want"]["status"].tolist() == [0, 0, 0] and made[p]["want"]["iters"].tolist() == [30, 30, 30]
    return made


def offset_view(t):
    """the same values one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def wide_rows(t, pad=3):
    """the same rows inside rows of E + pad floats, every second row of the buffer"""
    buf = torch.full(t.shape[:-2] + (2 * t.shape[-2], t.shape[-1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[..., 0::2, :t.shape[-1]]
    view.copy_(t)
    assert view.stride(-2) == 2 * (t.shape[-1] + pad) and not view.is_contiguous()
    return view


@pytest.mark.parametrize("p", [1, 2])
def test_contract_1_a_problem_depends_on_its_own_rows_only(batch, p):
    a, b, eps, want = batch["a"], batch["b"], batch[p]["eps"], batch[p]["want"]
    n_a, n_b, E = batch["shape"]
    assert same_outputs(run(offset_view(a), offset_view(b), eps, p), want)                          # alignment
    assert same_outputs(run(wide_rows(a), wide_rows(b), eps, p), want)                              # strides
    for q in range(3):                                                                              # alone, and in another place
        alone = run(a[q:q + 1], b[q:q + 1], eps[q:q + 1], p)
        assert all(same_bits(alone[k][0], want[k][q]) for k in OUT)
        assert same_outputs(run(a[q], b[q], eps[q:q + 1], p), alone)                                # [n, E]: one state
        assert same_outputs(run(a[q], b[q], float(eps[q].item()), p), alone)                        # a float epsilon
    order = [2, 0, 1, 0]
    moved = run(a[order], b[order], eps[order], p)
    assert all(same_bits(moved[k], want[k][order]) for k in OUT)
    shared = a[1:2].expand(3, n_a, E)                                                               # problem stride 0
    assert engine._swd_rows(shared, "a")[4] == 0
    copies = run(a[1:2].repeat(3, 1, 1), b, eps, p)
    assert same_outputs(run(shared, b, eps, p), copies) and same_outputs(run(a[1], b, eps, p), copies)
    assert same_outputs(run(a, b[2], eps, p), run(a, b[2:3].repeat(3, 1, 1), eps, p))
    lib = _hip.load()
    least, full = lib.dt_sinkhorn_workspace_bytes(1, n_a, n_b), lib.dt_sinkhorn_workspace_bytes(3, n_a, n_b)
    assert least < full
    for ws in (least, least + (full - least) // 2 + 8, full, 4 * full):                            # chunks of 1, 2, 3 and 3 problems
        assert same_outputs(run(a, b, eps, p, workspace_bytes=ws), want), ws
    with pytest.raises(ValueError):
        run(a, b, eps, p, workspace_bytes=least - 1)
    plain = engine.device_sinkhorn_ot(a, b, eps, p=p, max_iter=30, tol=0.0)                        # no potentials
    assert sorted(plain) == ["err", "iters", "ot", "status"] and same_outputs(plain, want, ("ot", "err", "iters", "status"))
    mc = engine.device_sinkhorn_mean_cost(a, b, p=p)
    assert same_outputs(engine.device_sinkhorn_mean_cost(wide_rows(a), offset_view(b), p=p, workspace_bytes=least), mc,
                        ("mean_cost", "status"))
    assert same_bits(engine.device_sinkhorn_mean_cost(a[2], b[2], p=p)["mean_cost"][0], mc["mean_cost"][2])


@pytest.mark.parametrize("p", [1, 2])
def test_contract_2_a_frozen_problem_has_the_bits_of_the_run_that_stops_there(batch, p):
    a, b, eps = batch["a"], batch["b"], batch[p]["eps"]
    stopped = run(a, b, eps, p, max_iter=500, tol=1e-6)
    iters = stopped["iters"].tolist()
    print(f"{ids(batch['shape'])} p={p}: frozen after {iters} steps, err {stopped['err'].tolist()}")
    assert stopped["status"].tolist() == [0, 0, 0] and all(1 < k < 500 for k in iters) and (stopped["err"] <= 1e-6).all()
    for q in range(3):
        fixed = run(a[q:q + 1], b[q:q + 1], eps[q:q + 1], p, max_iter=iters[q], tol=0.0)
        assert all(same_bits(fixed[k][0], stopped[k][q]) for k in OUT), q
        again = run(a[q:q + 1], b[q:q + 1], eps[q:q + 1], p, max_iter=iters[q], tol=1e-6)           # stops at the last step
        assert same_outputs(again, fixed)
    assert same_outputs(run(a, b, eps, p, max_iter=max(iters), tol=1e-6), stopped)


@pytest.mark.parametrize("p", [1, 2])
def test_contract_3_a_copy_is_the_set_itself(batch, p):
    a, eps = batch["a"], batch[p]["eps"]
    twin = a.clone()
    want = run(a, a, eps, p)
    for x, y in ((a, twin), (twin, twin), (twin, a), (offset_view(a), wide_rows(a))):
        assert same_outputs(run(x, y, eps, p), want)
    div = engine.device_sinkhorn_divergence(a, twin, eps, p=p, max_iter=30, tol=0.0)
    assert (div["divergence"] == 0).all() and not torch.signbit(div["divergence"]).any()
    assert same_bits(div["ot_ab"], want["ot"]) and same_bits(div["ot_aa"], want["ot"]) and same_bits(div["ot_bb"], want["ot"])
    assert torch.isfinite(want["ot"]).all() and not want["status"].any()


@pytest.mark.parametrize("p", [1, 2])
def test_contract_4_powers_of_two_scale_exactly(batch, p):
    a, b, eps, want = batch["a"], batch["b"], batch[p]["eps"], batch[p]["want"]
    mc = engine.device_sinkhorn_mean_cost(a, b, p=p)["mean_cost"]
    stopped = run(a, b, eps, p, max_iter=500, tol=1e-6)
    for k in (-3, 5):
        s, sp = 2.0 ** k, 2.0 ** (k * p)
        out = run(a * s, b * s, eps * sp, p)
        for key in ("ot", "f", "g"):
            assert same_bits(out[key], want[key] * sp), (key, k)
        assert same_bits(out["err"], want["err"]) and same_bits(out["iters"], want["iters"]) and not out["status"].any()
        assert same_bits(engine.device_sinkhorn_mean_cost(a * s, b * s, p=p)["mean_cost"], mc * sp)
        again = run(a * s, b * s, eps * sp, p, max_iter=500, tol=1e-6)
        assert same_bits(again["iters"], stopped["iters"]) and same_bits(again["err"], stopped["err"])
        assert same_bits(again["ot"], stopped["ot"] * sp)


def tree(v):
    """the header's tree over v padded with 0.0 to the next power of two, in float64"""
    n2 = 1
    while n2 < len(v):
        n2 *= 2
    part = np.zeros(n2)
    part[:len(v)] = v
    h = n2 // 2
    while h >= 1:
        part[:h] += part[h:2 * h]
        h //= 2
    return part[0]


@pytest.mark.parametrize("p", [1, 2])
def test_contract_5_the_potentials_are_what_the_value_was_made_from(batch, p):
    want = batch[p]["want"]
    f, g, ot = (want[k].cpu().numpy() for k in ("f", "g", "ot"))
    n_a, n_b, _ = batch["shape"]
    for q in range(3):
        assert ot[q] == tree(f[q]) / np.float64(n_a) + tree(g[q]) / np.float64(n_b)


# ------------------------------------------------------------------------------------------------ stopping rule
STOPS = [((64, 64, 48), 2, (2, 3, 4)), ((64, 64, 48), 1, (1, 2, 8)), ((37, 64, 19), 2, (4, 5, 8)), ((65, 130, 17), 1, (3, 4, 5))]


@pytest.mark.parametrize("shape,p,seeds", STOPS, ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_stopping_rule(shape, p, seeds):
    """tol = 1e-8 at rel_epsilon = 0.25.  The seeds are those for which the yardstick's err is above 2 tol at step k* - 1
    and below tol / 2 at step k*, so that the device, whose err is within a bound far below tol / 2 of it, must stop at k*."""
    n_a, n_b, E = shape
    tol = 1e-8
    pairs = [tuple(x[0] for x in ref.sets(seed, 1, n_a, n_b, E)) for seed in seeds]
    a, b = np.stack([x[0] for x in pairs]), np.stack([x[1] for x in pairs])
    eps = [ref.epsilon(a[q], b[q], p, 0.25) for q in range(3)]
    costs = [ref.cost(a[q], b[q], p) for q in range(3)]
    made = [ref.iterate(costs[q], eps[q], 100, tol=tol) for q in range(3)]
    stars = [r["iters"] for r in made]
    for q, r in enumerate(made):
        assert r["status"] == 0 and r["errs"][-2] > 2 * tol and r["errs"][-1] < tol / 2, (q, r["errs"][-2:])
        assert ref.forward_bound(costs[q], eps[q], r, E, p)["err"] < tol / 2
    da, db, de = dev(a), dev(b), dev(np.float64(eps))
    out = run(da, db, de, p, max_iter=100, tol=tol)
    print(f"{ids(shape)} p={p}: k* = {stars}, device iters {out['iters'].tolist()}, err {out['err'].tolist()}")
    assert out["iters"].tolist() == stars and (out["err"] <= tol).all() and out["status"].tolist() == [0, 0, 0]
    for q, r in enumerate(made):
        assert max(ratios(out, q, r, ref.forward_bound(costs[q], eps[q], r, E, p)).values()) <= 1.0
    short = run(da, db, de, p, max_iter=min(stars) - 1, tol=tol)
    assert short["status"].tolist() == [ref.NOT_CONVERGED] * 3 and short["iters"].tolist() == [min(stars) - 1] * 3
    assert (short["err"] > tol).all()
    for q in range(3):
        r = ref.iterate(costs[q], eps[q], min(stars) - 1, tol=tol)
        assert r["status"] == ref.NOT_CONVERGED
        assert max(ratios(short, q, r, ref.forward_bound(costs[q], eps[q], r, E, p)).values()) <= 1.0


# ------------------------------------------------------------------------------------------------ status
def flagged(out, q, bits):
    assert out["status"][q].item() == bits and out["iters"][q].item() == 0
    assert all(torch.isnan(out[k][q]).all() for k in ("ot", "err", "f", "g"))


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_a_nonfinite_row_flags_its_problem_only(batch, value):
    a, b, eps, want = batch["a"], batch["b"], batch[2]["eps"], batch[2]["want"]
    n_a, n_b, E = batch["shape"]
    mc = engine.device_sinkhorn_mean_cost(a, b)
    for side, (x, n) in enumerate(((a, n_a), (b, n_b))):
        bad = x.clone()
        bad[1, n - 1, E - 1] = value
        out = run(bad, b, eps) if side == 0 else run(a, bad, eps)
        flagged(out, 1, ref.NONFINITE)
        assert all(same_bits(out[k][[0, 2]], want[k][[0, 2]]) for k in OUT)
        got = engine.device_sinkhorn_mean_cost(bad, b) if side == 0 else engine.device_sinkhorn_mean_cost(a, bad)
        assert got["status"].tolist() == [0, 1, 0] and torch.isnan(got["mean_cost"][1])
        assert same_bits(got["mean_cost"][[0, 2]], mc["mean_cost"][[0, 2]])
    bad = a.clone()
    bad[1, 0, 0] = value
    both = eps.clone()
    both[1] = -1.0
    flagged(run(bad, b, both), 1, ref.NONFINITE | ref.BAD_EPS)
    div = engine.device_sinkhorn_divergence(bad, b, eps, max_iter=30, tol=0.0)
    assert div["status"].tolist() == [0, 1, 0] and torch.isnan(div["divergence"][1]) and torch.isfinite(div["divergence"][[0, 2]]).all()


@pytest.mark.parametrize("value", [0.0, -1.0, float("inf"), float("-inf"), float("nan")])
def test_a_bad_epsilon_flags_its_problem_only(batch, value):
    a, b, eps, want = batch["a"], batch["b"], batch[2]["eps"], batch[2]["want"]
    bad = eps.clone()
    bad[1] = value
    out = run(a, b, bad)
    flagged(out, 1, ref.BAD_EPS)
    assert all(same_bits(out[k][[0, 2]], want[k][[0, 2]]) for k in OUT)
    stopped = run(a, b, bad, max_iter=500, tol=1e-6)
    flagged(stopped, 1, ref.BAD_EPS)
    assert stopped["status"][[0, 2]].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ the Python layers
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_divergence_of_a_clone_is_zero_and_of_two_draws_is_positive(shape):
    n_a, n_b, E = shape
    a, b = (dev(x[0]) for x in ref.sets(7 + n_a + n_b + E, 1, n_a, n_b, E))
    eps = ref.epsilon(a.cpu().numpy(), b.cpu().numpy(), 2, 0.25)
    zero = engine.device_sinkhorn_divergence(a, a.clone(), eps, max_iter=60)             # (converged or not: the same bits thrice)
    assert zero["divergence"].tolist() == [0.0] and zero["status"].item() & (ref.NONFINITE | ref.BAD_EPS) == 0
    out = engine.device_sinkhorn_divergence(a, b, eps, max_iter=200, tol=1e-9)          # (a self term may take longer: bit 4)
    assert out["status"].item() & (ref.NONFINITE | ref.BAD_EPS) == 0
    assert out["divergence"].item() >= 0 and (n_a == n_b == 1 or out["divergence"].item() > 0)
    assert same_bits(out["divergence"], out["ot_ab"] - (0.5 * out["ot_aa"] + 0.5 * out["ot_bb"]))
    aa = engine.device_sinkhorn_ot(a, a, eps, max_iter=200, tol=1e-9)
    for given in (aa, aa["ot"]):                                                                     # a self term made before
        again = engine.device_sinkhorn_divergence(a, b, eps, max_iter=200, tol=1e-9, self_a=given)
        assert all(same_bits(again[k], out[k]) for k in ("divergence", "ot_ab", "ot_aa", "ot_bb"))
    swapped = engine.device_sinkhorn_divergence(b, a, eps, max_iter=200, tol=1e-9, self_b=aa)
    assert same_bits(swapped["ot_bb"], out["ot_aa"]) and same_bits(swapped["ot_aa"], out["ot_bb"])


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_divergence_is_symmetric_at_convergence(shape):
    """S(a, b) against S(b, a) with tol = 1e-11 and at most 2000 steps, on all ten shapes.  The self terms of the two are
    the same two problems, so they cancel bit for bit and only OT(a, b) and OT(b, a) differ: by their rounding (the forward
    bounds of the yardstick's runs) and by what the steps have left.  The dual objective is concave with gradient
    (a - row marginal, b - column marginal), whose L1 norm does not grow along the steps and is err at the last step run,
    and the potentials are within 2 F of the limit's in the max norm (F the largest |f|, |g| met), so a term is within
    2 F err of its limit, on the device and in the yardstick alike (they may stop one step apart): 4 F max(err, tol)
    between the two.
    Where a set has more than 130 rows (2048 x 3, 3 x 2048, 200 x 200 x 768) the self terms are made once on the device
    with 200 steps and handed to both calls -- 2000 steps on a 2048 x 2048 matrix, twice, is not a test of seconds, and the
    yardstick would need minutes for it -- so there the value S(a, b) itself is not held against the yardstick, only the
    symmetry, for which the yardstick's runs of (a, b) and (b, a) suffice."""
    n_a, n_b, E = shape
    small = shape in SMALL
    a, b = (x[0] for x in ref.sets(11 + n_a + n_b + E, 1, n_a, n_b, E))
    eps, tol = ref.epsilon(a, b, 2, 0.25), 1e-11
    runs = {}
    for name, (x, y) in {"ab": (a, b), "ba": (b, a), "aa": (a, a), "bb": (b, b)}.items():
        if small or name in ("ab", "ba"):
            C = ref.cost(x, y, 2)
            r = ref.iterate(C, eps, 2000, tol=tol)
            runs[name] = (r, ref.forward_bound(C, eps, r, E, 2)["ot"] + 4 * r["F"] * max(float(r["err"]), tol))
    assert runs["ab"][0]["status"] == runs["ba"][0]["status"] == 0
    da, db = dev(a), dev(b)
    kw = dict(max_iter=2000, tol=tol)
    if small:
        ab = engine.device_sinkhorn_divergence(da, db, eps, **kw)
        ba = engine.device_sinkhorn_divergence(db, da, eps, **kw)
    else:
        aa, bb = (engine.device_sinkhorn_ot(x, x, eps, max_iter=200, tol=tol) for x in (da, db))
        ab = engine.device_sinkhorn_divergence(da, db, eps, self_a=aa, self_b=bb, **kw)
        ba = engine.device_sinkhorn_divergence(db, da, eps, self_a=bb, self_b=aa, **kw)
    assert ab["status"].item() & 3 == ba["status"].item() & 3 == 0
    assert same_bits(ab["ot_aa"], ba["ot_bb"]) and same_bits(ab["ot_bb"], ba["ot_aa"])
    d_ab, d_ba = ab["divergence"].item(), ba["divergence"].item()
    largest = max(abs(ab[k].item()) for k in ("ot_ab", "ot_aa", "ot_bb"))
    print(f"{ids(shape)}: S(a,b)={d_ab:.12g} S(b,a)={d_ba:.12g} |difference| {abs(d_ab - d_ba):.3g} "
          f"summed bounds {runs['ab'][1] + runs['ba'][1]:.3g}")
    assert d_ab >= 0 and d_ba >= 0
    assert abs(d_ab - d_ba) <= runs["ab"][1] + runs["ba"][1] + 4 * ref.U * largest
    if small:
        slack = ref.divergence_bound(runs["ab"][1], runs["aa"][1], runs["bb"][1], largest)
        want = ref.divergence(runs["ab"][0]["ot"], runs["aa"][0]["ot"], runs["bb"][0]["ot"])
        print(f"{ids(shape)}: yardstick {float(want):.12g} slack {slack:.3g}")
        assert abs(ref.LD(d_ab) - want) <= slack


# ------------------------------------------------------------------------------------------------ the order of the sums
def lane_butterfly(v):
    """the header's sum of a row: lane l of 64 adds v[l], v[l + 64], .. from 0.0, then s += s(lane ^ m), m = 32 .. 1"""
    s = np.zeros(64)
    for j0 in range(0, len(v), 64):
        chunk = v[j0:j0 + 64]
        s[:len(chunk)] += chunk
    m = 32
    while m >= 1:
        s = s + s[np.arange(64) ^ m]
        m //= 2
    assert (s == s[0]).all()
    return s[0]


@pytest.mark.parametrize("shape", [(5, 3, 7), (37, 130, 7), (70, 200, 3)], ids=ids)
def test_mean_cost_has_the_bits_of_the_header_s_order_restated_in_numpy(shape):
    """p = 2, where nothing transcendental enters: every cell as the chain acc = fma(d, d, acc) over e ascending (each
    fused multiply-add from exact rationals, rounded once), every row by lanes and butterfly, the rows by the tree, one
    division -- restated here from the header's words alone, and compared bit for bit.  (The sums of the half-steps add
    the device's exp values in these same orders -- the row pass through the same lanes and butterfly -- but cannot be
    restated to the bit on the host, whose exp is another.)"""
    from fractions import Fraction
    n_a, n_b, E = shape
    a, b = (x[0] for x in ref.sets(3 + n_a + n_b + E, 1, n_a, n_b, E))
    C = np.zeros((n_a, n_b))
    for i in range(n_a):
        for j in range(n_b):
            acc = 0.0
            for e in range(E):
                d = float(a[i, e]) - float(b[j, e])
                acc = float(Fraction(d) * Fraction(d) + Fraction(acc))
            C[i, j] = acc
    want = tree(np.array([lane_butterfly(C[i]) for i in range(n_a)])) / np.float64(n_a * n_b)
    got = engine.device_sinkhorn_mean_cost(dev(a), dev(b), p=2)["mean_cost"].item()
    assert got == want, (got, want)
    other = C.sum() / (n_a * n_b)                                             # numpy's own order: close, and (mostly) other bits
    assert abs(other - want) <= 64 * ref.U * want


def trajectory_pair(models, S=4, T=2):
    from distillation_trajectories_amd.analysis.trajectory_engine import sample_grid
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model, noise_table
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, T
    teacher = copy.deepcopy(models(0.1)).to(DEV).eval()
    student = make_model(DiffusionUNet, cfg, 0.1, seed=4321).to(DEV).eval()        # the same width, other weights
    table = noise_table(42, S + T - 1, (1, 3, 16, 16)).reshape(S + T - 1, -1).to(DEV)
    return [sample_grid(engine.UNetHandle.for_module(m), table, 0, S, T, [None], 16, 16)[None] for m in (teacher, student)]


@pytest.mark.parametrize("p", [1, 2])
def test_trajectories(models, p):
    """3 states, 4 samples, 16 x 16: the pair form against the engine calls it is made of, and the list forms"""
    X, Y = trajectory_pair(models)
    assert X.shape == (3, 4, 768)
    res = sk.sinkhorn_pairs(X, Y, p=p)
    mc = engine.device_sinkhorn_mean_cost(X, X, p=p)["mean_cost"]
    eps = mc * 0.05
    want = engine.device_sinkhorn_divergence(X, Y, eps, p=p)
    assert np.array_equal(res["epsilon"], eps.cpu().numpy()) and (res["epsilon"] > 0).all()
    assert np.array_equal(res["divergence"], want["divergence"].cpu().numpy()) and res["divergence"].dtype == np.float64
    assert res["ot"].shape == (3, 3) and np.array_equal(res["ot"][:, 1], want["ot_aa"].cpu().numpy())
    print(f"p={p}: iters {res['iters'].tolist()} err {res['err'].tolist()} status {res['status'].tolist()}")
    assert not (res["status"] & 3).any() and res["iters"].shape == res["err"].shape == (3,) and (res["iters"] >= 1).all()
    assert res["divergence"][0] == 0 and (res["divergence"][1:] > 0).all()                       # the shared start noise
    C = ref.cost(X[2].cpu().numpy(), X[2].cpu().numpy(), p)
    assert abs(ref.LD(mc[2].item()) - C.mean()) <= ref.mean_cost_bound(C, 768, p)
    given = sk.sinkhorn_pairs(X, Y, epsilon=float(res["epsilon"][1]), p=p)
    assert given["divergence"][1] == res["divergence"][1] and (given["epsilon"] == res["epsilon"][1]).all()
    lists = [[x.reshape(4, 3, 16, 16).cpu() for x in X], [(y.reshape(4, 3, 16, 16), 2 - i) for i, y in enumerate(Y)]]
    again = sk.sinkhorn_trajectories(*lists, p=p)
    for key in res:
        assert np.array_equal(again[key], res[key]), key
    with pytest.raises(ValueError):
        sk.sinkhorn_trajectories(lists[0], lists[1][:2])


def test_sweep_tiny(models, tmp_path):
    """sf 0.1 (the teacher's own module) and 0.2, 16 x 16, T = 2, 4 samples"""
    from distillation_trajectories_amd.analysis.trajectory_engine import sample_grid
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.synthetic import noise_table
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 2
    teacher = copy.deepcopy(models(0.1)).to(DEV).eval()
    student = copy.deepcopy(models(0.2)).to(DEV).eval()
    scales = [None, 3.0]
    res = sk.sinkhorn_sweep(teacher, [teacher, student], cfg, scales, 4, output_dir=str(tmp_path))
    keys = ("divergence", "divergence_split", "floor", "ot", "epsilon", "err", "iters", "status")
    for key in keys:
        assert res[key].shape == ((2, 2, 3, 3) if key == "ot" else (2, 2, 3)), key
    assert sorted(res) == sorted(keys + ("states", "guidance_scales"))
    assert res["states"].tolist() == [0, 1, 2] and np.isnan(res["guidance_scales"][0]) and res["guidance_scales"][1] == 3.0
    print(f"iters {res['iters'].tolist()} status {res['status'].tolist()}")
    assert not (res["status"] & 3).any() and (res["epsilon"] > 0).all() and (res["iters"] >= 1).all()
    assert np.isfinite(res["floor"]).all() and (res["floor"] > 0).all()
    assert np.array_equal(res["floor"][0], res["floor"][1])                                    # it does not depend on the student
    assert (res["divergence"][0] == 0).all()                                                   # a student that is the teacher
    assert np.array_equal(res["divergence_split"][0], res["floor"][0])                         # ... and whose split is the floor
    assert (res["divergence"][1][:, 1:] > 0).all() and (res["divergence_split"][1] > 0).all()
    assert (res["divergence"][1][:, 0] == 0).all()                                             # the shared start noise
    assert np.array_equal(res["epsilon"][0], res["epsilon"][1])                                # the teacher's, whoever the student
    for k in range(2):
        with np.load(os.path.join(str(tmp_path), f"sinkhorn_student_{k}.npz")) as f:
            assert sorted(f.files) == sorted(res)
            for key in keys:
                assert np.array_equal(f[key], res[key][k]), key
            assert f["states"].tolist() == [0, 1, 2]
    # one cell run alone: (student 1, scale 3.0)
    table = noise_table(42, 4 + 2 - 1, (1, 3, 16, 16)).reshape(5, -1).to(DEV)
    X, Y = (sample_grid(engine.UNetHandle.for_module(m), table, 0, 4, 2, [3.0], 16, 16)[3.0] for m in (teacher, student))
    alone = sk.sinkhorn_pairs(X, Y)
    for key in ("divergence", "ot", "epsilon", "err", "iters", "status"):
        assert np.array_equal(alone[key], res[key][1][1]), key
    assert np.array_equal(sk.sinkhorn_pairs(X[:, 0::2], Y[:, 1::2])["divergence"], res["divergence_split"][1][1])
    assert np.array_equal(sk.sinkhorn_pairs(X[:, 0::2], X[:, 1::2])["divergence"], res["floor"][1][1])
    every = sk.sinkhorn_sweep(teacher, [student], cfg, [3.0], 4, every=2, p=1, output_dir=str(tmp_path / "every"))
    assert every["states"].tolist() == [0, 2] and every["divergence"].shape == (1, 1, 2)
    assert np.array_equal(every["divergence"][0][0], sk.sinkhorn_pairs(X[[0, 2]], Y[[0, 2]], p=1)["divergence"])
