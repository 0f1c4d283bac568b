"""GPU: the sliced Wasserstein distance (include/dt_hip_swd.h, engine.device_swd / device_swd_sorted,
analysis/metrics/sliced_wasserstein.py) against the extended-precision yardstick tests/swd_ref64.py within the bounds derived
there, the header's seven bit contracts, the status words and the analysis layer.  Observed error over bound on an MI355X:
DESIGN §9ag."""
import copy
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import swd_ref64 as ref
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.analysis.metrics import sliced_wasserstein as sw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (2, 2), (5, 5), (7, 3), (3, 7), (64, 48), (256, 256), (2048, 1)]
WIDTHS = [1, 3, 5, 64, 768]
COUNTS = [1, 3, 64, 65]
OUT = ("w", "mean_w", "max_w", "argmax")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t) for t in (a, b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.int64), b.view(np.int64)) if a.dtype == np.float64 else np.array_equal(a, b)


def same_outputs(x, y, keys=OUT + ("status",)):
    return all(same_bits(x[k], y[k]) for k in keys)


def run(a, b, theta, p=2, **kw):
    return engine.device_swd(a, b, directions=theta, p=p, per_direction=True, **kw)


def ratios(out, made, bound):
    """the largest |device - yardstick| / bound of w, mean_w and max_w; asserts the argmax is a maximum within the bound"""
    worst = {}
    for key in ("w", "mean_w", "max_w"):
        err, tol = np.abs(out[key].astype(ref.LD) - made[key]), bound[key]
        worst[key] = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
        assert (err[tol == 0] == 0).all(), key
    picked = np.take_along_axis(made["w"], out["argmax"][..., None].astype(np.int64), axis=-1)[..., 0]
    assert (picked >= made["max_w"] - 2 * bound["max_w"]).all()
    return worst


# ------------------------------------------------------------------------------------------------ tolerance
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("n_a,n_b", SIZES)
def test_outputs_within_the_forward_bound(n_a, n_b, E, kind):
    """L in {1, 3, 64, 65} (the leading directions of one table), P in {1, 3} (the leading problems of one batch), p in {1, 2}"""
    a, b = ref.sets(1000 * n_a + 10 * n_b + E, 3, n_a, n_b, E, kind)
    theta = ref.unit_directions(E + 1, max(COUNTS), E)
    case = ref.Case(a, b, theta)
    da, db, dt = dev(a), dev(b), dev(theta)
    worst = dict.fromkeys(("w", "mean_w", "max_w"), 0.0)
    for p in (1, 2):
        for L in COUNTS:
            made, bound = case.swd(p, L), case.forward_bound(p, L)
            for P in (1, 3):
                out = host(run(da[:P], db[:P], dt[:L], p))
                assert not out["status"].any() and out["w"].shape == (P, L) and out["mean_w"].shape == (P,)
                got = ratios(out, {k: v[:P] for k, v in made.items()}, {k: v[:P] for k, v in bound.items()})
                worst = {k: max(worst[k], got[k]) for k in worst}
    print(f"({n_a},{n_b}) E={E} {kind}: error / bound " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("p", [1, 2])
def test_largest_sets_within_the_forward_bound(p):
    a, b = ref.sets(7, 1, 2048, 2048, 64, "gauss")
    theta = ref.unit_directions(8, 4, 64)
    case = ref.Case(a, b, theta)
    worst = ratios(host(run(dev(a), dev(b), dev(theta), p)), case.swd(p), case.forward_bound(p))
    print(f"(2048,2048) E=64 L=4 p={p}: error / bound " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


# ------------------------------------------------------------------------------------------------ contracts
@pytest.fixture(scope="module", params=[(7, 3, 5, 3), (5, 5, 3, 4), (130, 48, 37, 65)], ids=lambda s: "x".join(map(str, s)))
def batch(request):
    """3 problems on contiguous tensors and their outputs for both p: what every variation below has to reproduce"""
    n_a, n_b, E, L = request.param
    a, b = ref.sets(n_a + E, 3, n_a, n_b, E, "gauss")
    theta = ref.unit_directions(L, L, E)
    a, b, theta = dev(a), dev(b), dev(theta)
    return {"a": a, "b": b, "theta": theta, "shape": request.param, 1: run(a, b, theta, 1), 2: run(a, b, theta, 2)}


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
    a, b, theta, want = batch["a"], batch["b"], batch["theta"], batch[p]
    n_a, n_b, E, L = batch["shape"]
    assert same_outputs(run(offset_view(a), offset_view(b), offset_view(theta), p), want)          # alignment
    assert same_outputs(run(wide_rows(a), wide_rows(b), wide_rows(theta), p), want)                # strides
    for q in range(3):                                                                             # alone, and in another place
        alone = run(a[q:q + 1], b[q:q + 1], theta, p)
        assert all(same_bits(alone[k][0], want[k][q]) for k in OUT)
        flat = run(a[q], b[q], theta, p)                                                           # [n, E]: one state
        assert same_outputs(flat, alone)
    order = [2, 0, 1, 0]
    moved = run(a[order], b[order], theta, p)
    assert all(same_bits(moved[k], want[k][order]) for k in OUT)
    shared = run(a[1:2].expand(3, n_a, E), b, theta, p)                                            # problem stride 0
    assert shared is not None and engine._swd_rows(a[1:2].expand(3, n_a, E), "a")[4] == 0
    copies = run(a[1:2].repeat(3, 1, 1), b, theta, p)
    assert same_outputs(shared, copies) and same_outputs(run(a[1], b, theta, p), copies)
    assert same_outputs(run(a, b[2], theta, p), run(a, b[2:3].repeat(3, 1, 1), theta, p))
    lib = _hip.load()
    least, full = lib.dt_swd_workspace_bytes(1, n_a, n_b, L), lib.dt_swd_workspace_bytes(3, n_a, n_b, L)
    assert least < full
    for ws in (least, least + (full - least) // 2 + 8, full, 4 * full):                           # chunks of 1, 2, 3 and 3 problems
        assert same_outputs(run(a, b, theta, p, workspace_bytes=ws), want), ws
    with pytest.raises(ValueError):
        run(a, b, theta, p, workspace_bytes=least - 1)
    assert same_outputs(engine.device_swd(a, b, directions=theta, p=p), want, ("mean_w", "max_w", "argmax", "status"))   # no w


@pytest.mark.parametrize("p", [1, 2])
def test_contracts_2_and_3_row_order_and_the_order_of_the_sets(batch, p):
    a, b, theta, want = batch["a"], batch["b"], batch["theta"], batch[p]
    gen = torch.Generator().manual_seed(5)
    pa, pb = torch.randperm(a.shape[1], generator=gen).to(DEV), torch.randperm(b.shape[1], generator=gen).to(DEV)
    assert same_outputs(run(a[:, pa], b[:, pb], theta, p), want)
    assert same_outputs(run(a.flip(1), b, theta, p), want)
    assert same_outputs(run(b, a, theta, p), want)


@pytest.mark.parametrize("p", [1, 2])
def test_contract_4_a_copy_or_a_permutation_is_at_distance_zero(batch, p):
    a, theta = batch["a"], batch["theta"]
    perm = torch.randperm(a.shape[1], generator=torch.Generator().manual_seed(6)).to(DEV)
    for other in (a.clone(), a[:, perm], a.flip(1)):
        out = host(run(a, other, theta, p))
        for key in ("w", "mean_w", "max_w"):
            assert (out[key] == 0).all() and not np.signbit(out[key]).any(), key
        assert (out["argmax"] == 0).all() and not out["status"].any()


@pytest.mark.parametrize("p", [1, 2])
def test_contract_5_powers_of_two_scale_exactly(batch, p):
    a, b, theta, want = batch["a"], batch["b"], batch["theta"], batch[p]
    for k in (-3, 5):
        out = run(a * 2.0 ** k, b * 2.0 ** k, theta, p)
        for key in ("w", "mean_w", "max_w"):
            assert same_bits(out[key], want[key] * 2.0 ** (k * p)), (key, k)
        assert same_bits(out["argmax"], want["argmax"])


@pytest.mark.parametrize("p", [1, 2])
def test_contract_6_sorted_then_distance_is_the_single_call(batch, p):
    a, b, theta, want = batch["a"], batch["b"], batch["theta"], batch[p]
    n_a, n_b, E, L = batch["shape"]
    sa, sb = engine.device_swd_sorted(a, theta), engine.device_swd_sorted(b, theta)
    assert sa.sorted.shape == (3, L, n_a) and sb.sorted.shape == (3, L, n_b) and not sa.status.any() and sa.n == n_a
    assert (sa.sorted[..., 1:] >= sa.sorted[..., :-1]).all() and (sb.sorted[..., 1:] >= sb.sorted[..., :-1]).all()
    proj = np.sort(ref.project(theta.cpu().numpy(), a.cpu().numpy()), axis=-1)
    assert (np.abs(sa.sorted.cpu().numpy() - proj) <= ref.delta(theta.cpu().numpy(), a.cpu().numpy())[..., None]).all()
    for x, y in ((sa, sb), (sa, b), (a, sb)):
        assert same_outputs(engine.device_swd(x, y, p=p, per_direction=True), want)
    assert same_outputs(engine.device_swd(sa, sb, directions=theta, p=p, per_direction=True), want)
    # a shared teacher: one sorted set against three, and three copies of it
    one = engine.device_swd_sorted(a[1], theta)
    assert one.sorted.shape == (1, L, n_a) and same_bits(one.sorted[0], sa.sorted[1])
    copies = run(a[1:2].repeat(3, 1, 1), b, theta, p)
    assert same_outputs(engine.device_swd(one, sb, p=p, per_direction=True), copies)
    assert same_outputs(engine.device_swd(one, b, p=p, per_direction=True), copies)
    assert same_outputs(engine.device_swd(sb, one, p=p, per_direction=True), copies)
    with pytest.raises(ValueError, match="other directions"):
        engine.device_swd(sa, b, directions=theta.clone(), p=p)
    with pytest.raises(ValueError, match="other directions"):
        engine.device_swd(sa, engine.device_swd_sorted(b, theta.clone()), p=p)


@pytest.mark.parametrize("n_a,n_b,E", [(7, 3, 5), (5, 5, 3), (130, 48, 37), (64, 64, 16), (2048, 1, 2)])
@pytest.mark.parametrize("p", [1, 2])
def test_contract_7_integer_data_on_the_axes_is_exact(n_a, n_b, E, p):
    """rows of integers in [-9, 9], directions e_0 .. e_{E-1}: w = T / (nB nS) and mean_w = sum T / (nB nS L), correctly rounded"""
    rng = np.random.RandomState(n_a + n_b + E)
    a, b = rng.randint(-9, 10, (2, n_a, E)), rng.randint(-9, 10, (2, n_b, E))
    theta = np.eye(E, dtype=np.float32)
    out = host(run(dev(a.astype(np.float32)), dev(b.astype(np.float32)), dev(theta), p))
    big, small = (a, b) if n_a >= n_b else (b, a)
    i, j, wt = ref.overlaps(big.shape[1], small.shape[1])
    sb_, ss_ = np.sort(big, axis=1), np.sort(small, axis=1)                       # [2, n, E]: column e is direction e
    totals = (wt[None, :, None] * np.abs(sb_[:, i] - ss_[:, j]) ** p).sum(axis=1)   # [2, E] int64, exact
    for q in range(2):
        w = [Fraction(int(t), n_a * n_b) for t in totals[q]]
        assert out["w"][q].tolist() == [float(x) for x in w]
        assert out["mean_w"][q] == float(Fraction(int(totals[q].sum()), n_a * n_b * E))
        assert out["max_w"][q] == float(max(w)) and out["argmax"][q] == w.index(max(w))
    assert not out["status"].any()


# ------------------------------------------------------------------------------------------------ status
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_a_nonfinite_row_flags_its_problem_only(batch, value):
    a, b, theta, want = batch["a"], batch["b"], batch["theta"], batch[2]
    n_a, n_b, E, L = batch["shape"]
    for side, (x, n) in enumerate(((a, n_a), (b, n_b))):
        bad = x.clone()
        bad[1, n - 1, E - 1] = value
        out = run(bad, b, theta) if side == 0 else run(a, bad, theta)
        assert out["status"].tolist() == [0, 1, 0] and out["argmax"][1].item() == -1
        for key in ("w", "mean_w", "max_w"):
            assert torch.isnan(out[key][1]).all(), key
            assert same_bits(out[key][[0, 2]], want[key][[0, 2]]), key
        assert same_bits(out["argmax"][[0, 2]], want["argmax"][[0, 2]])
        made = engine.device_swd_sorted(bad, theta)
        assert made.status.tolist() == [0, 1, 0] and torch.isnan(made.sorted[1]).all() and torch.isfinite(made.sorted[[0, 2]]).all()
        other = engine.device_swd(made, a if side else b, p=2, per_direction=True)
        assert same_outputs(other, out)
    for l, e in ((0, 0), (L - 1, E - 1)):                                        # anywhere in theta: every problem
        poisoned = theta.clone()
        poisoned[l, e] = value
        out = run(a, b, poisoned)
        assert out["status"].tolist() == [1, 1, 1] and (out["argmax"] == -1).all()
        assert all(torch.isnan(out[key]).all() for key in ("w", "mean_w", "max_w"))
        assert engine.device_swd_sorted(a, poisoned).status.tolist() == [1, 1, 1]


# ------------------------------------------------------------------------------------------------ the analysis layer
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
    grids = [sample_grid(engine.UNetHandle.for_module(m), table, 0, S, T, [None], 16, 16)[None] for m in (teacher, student)]
    return grids


@pytest.mark.parametrize("p", [1, 2])
def test_trajectories_against_the_yardstick(models, p):
    """3 states, 4 samples, 16 x 16, 16 directions: swd and max_swd within the bound, carried through the p-th root:
    |m^(1/p) - r^(1/p)| <= |m - r| / r^(1 - 1/p), and one rounding of the root"""
    X, Y = trajectory_pair(models)
    assert X.shape == (3, 4, 768)
    res = sw.sliced_wasserstein_pairs(X, Y, n_directions=16, p=p)
    theta = engine.swd_directions(768, 16, 0).numpy()
    assert np.array_equal(res["directions"], theta) and res["swd"].shape == res["max_swd"].shape == (3,)
    assert res["swd"].dtype == np.float64 and not res["status"].any() and res["status"].shape == res["argmax"].shape == (3,)
    case = ref.Case(X.cpu().numpy(), Y.cpu().numpy(), theta)
    made, bound = case.swd(p), case.forward_bound(p)
    for key, name in (("swd", "mean_w"), ("max_swd", "max_w")):
        want = made[name] ** (ref.LD(1) / p)
        has = made[name] > 0
        tol = np.where(has, bound[name] / np.where(has, made[name], 1) ** (1 - ref.LD(1) / p), 0) + 2 * ref.U * want
        assert (np.abs(res[key].astype(ref.LD) - want) <= tol).all(), key
    assert res["swd"][0] == 0 and res["max_swd"][0] == 0 and res["argmax"][0] == 0              # the shared start noise
    assert (res["swd"][1:] > 0).all() and (res["max_swd"] >= res["swd"]).all()
    lists = [[x.reshape(4, 3, 16, 16).cpu() for x in X], [(y.reshape(4, 3, 16, 16), 2 - i) for i, y in enumerate(Y)]]
    again = sw.sliced_wasserstein_trajectories(*lists, n_directions=16, p=p)
    for key in res:
        assert np.array_equal(again[key], res[key]), key
    with pytest.raises(ValueError):
        sw.sliced_wasserstein_trajectories(lists[0], lists[1][:2])


def test_sweep_tiny(models, tmp_path):
    """sf 0.1 (the teacher's own module) and 0.2, 16 x 16, T = 4, 8 samples, 16 directions"""
    from distillation_trajectories_amd.analysis.trajectory_engine import sample_grid
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.synthetic import noise_table
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 4
    teacher = copy.deepcopy(models(0.1)).to(DEV).eval()
    student = copy.deepcopy(models(0.2)).to(DEV).eval()
    scales = [None, 3.0]
    res = sw.sliced_wasserstein_sweep(teacher, [teacher, student], cfg, scales, 8, n_directions=16, output_dir=str(tmp_path))
    keys = ("swd", "swd_split", "floor", "max_swd", "argmax", "status")
    for key in keys:
        assert res[key].shape == (2, 2, 5), key
    assert res["states"].tolist() == [0, 1, 2, 3, 4] and res["directions"].shape == (16, 768)
    assert np.isnan(res["guidance_scales"][0]) and res["guidance_scales"][1] == 3.0 and not res["status"].any()
    assert np.isfinite(res["floor"]).all() and (res["floor"] >= 0).all() and (res["floor"][:, :, 1:] > 0).all()
    assert np.array_equal(res["floor"][0], res["floor"][1])                                    # it does not depend on the student
    assert (res["swd"][0] == 0).all() and (res["max_swd"][0] == 0).all()                       # a student that is the teacher
    assert np.array_equal(res["swd_split"][0], res["floor"][0])                                # ... and whose split is the floor
    assert (res["swd"][1][:, 1:] > 0).all() and (res["swd_split"][1] > 0).all()
    assert (res["swd"][1][:, 0] == 0).all()                                                    # the shared start noise
    assert not np.array_equal(res["swd"][1][0], res["swd"][1][1])                              # the scales differ
    for k in range(2):
        with np.load(os.path.join(str(tmp_path), f"swd_student_{k}.npz")) as f:
            assert sorted(f.files) == sorted(res)
            for key in keys:
                assert np.array_equal(f[key], res[key][k]), key
            assert np.array_equal(f["directions"], res["directions"]) and f["states"].tolist() == [0, 1, 2, 3, 4]
    # one cell run alone: (student 1, scale 3.0)
    table = noise_table(42, 8 + 4 - 1, (1, 3, 16, 16)).reshape(11, -1).to(DEV)
    X, Y = (sample_grid(engine.UNetHandle.for_module(m), table, 0, 8, 4, [3.0], 16, 16)[3.0] for m in (teacher, student))
    alone = sw.sliced_wasserstein_pairs(X, Y, n_directions=16)
    for key in ("swd", "max_swd", "argmax", "status"):
        assert np.array_equal(alone[key], res[key][1][1]), key
    assert np.array_equal(sw.sliced_wasserstein_pairs(X[:, 0::2], Y[:, 1::2], n_directions=16)["swd"], res["swd_split"][1][1])
    assert np.array_equal(sw.sliced_wasserstein_pairs(X[:, 0::2], X[:, 1::2], n_directions=16)["swd"], res["floor"][1][1])
    every = sw.sliced_wasserstein_sweep(teacher, [student], cfg, [3.0], 8, every=3, n_directions=16, p=1,
                                        output_dir=str(tmp_path / "every"))
    assert every["states"].tolist() == [0, 3, 4] and every["swd"].shape == (1, 1, 3)
    assert np.array_equal(every["swd"][0][0], sw.sliced_wasserstein_pairs(X[[0, 3, 4]], Y[[0, 3, 4]], n_directions=16, p=1)["swd"])
