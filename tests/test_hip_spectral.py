"""GPU: spatial-frequency spectra (include/dt_hip_spectral.h, engine.device_spectrum / device_spectral_pair,
analysis/metrics/spectral.py) against the extended-precision yardstick tests/spectral_ref64.py within the tolerances derived
there, and the header's five bit contracts.  Observed error over bound on an MI355X: DESIGN §9af."""
import copy
import os

import numpy as np
import pytest
import torch

import spectral_ref64 as ref
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.analysis.metrics import spectral

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 2), (3, 5), (16, 16), (28, 28), (64, 64), (64, 7), (1, 64)]
KINDS = ("gauss", "offset", "near")
KEYS = ("power_a", "power_b", "cross", "error")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def rows(x):
    """[..., C, H, W] numpy -> device [..., E]"""
    return dev(x).flatten(-3)


def stacked(out):
    """the five values per bin of a pair result, [..., C, n_bins, 5] float64 on the host, in the header's order"""
    return torch.cat([out["power_a"].unsqueeze(-1), out["power_b"].unsqueeze(-1), out["cross"], out["error"].unsqueeze(-1)],
                     dim=-1).cpu().numpy()


def pair(a, b, bins=None, **kw):
    C, H, W = a.shape[-3:]
    return engine.device_spectral_pair(rows(a), rows(b), C, H, W, bins=bins, **kw)


def same_bits(a, b):
    a, b = (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t) for t in (a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def tables(H, W):
    """{name: (the ``bins`` argument, the table the yardstick uses, n_bins)}"""
    table, cells = engine.radial_bins(H, W)
    holes, n_holes = ref.holes_table(H, W)
    out = {"radial": (None, table, len(cells)), "holes": (holes, holes, n_holes)}
    if (H, W) in ((3, 5), (16, 16)):               # 16 x 16: DT_SPECTRAL_MAX_BINS bins
        each, n_each = ref.cell_table(H, W)
        out["cells"] = (each, each, n_each)
    return out


# ------------------------------------------------------------------------------------------------ tolerance
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_outputs_within_the_forward_bound(H, W, C):
    """all five outputs, three kinds of input, the radial table, one with left-out cells and (3 x 5, 16 x 16) one bin
    per coefficient; 3 x 2 rows"""
    worst = dict.fromkeys(ref.NAMES, 0.0)
    for k, kind in enumerate(KINDS):
        a, b = ref.pictures(100 * H + W + 7 * C + k, (3, 2, C, H, W), kind)
        made = ref.spectra(a, b)
        for name, (bins, table, n_bins) in tables(H, W).items():
            out = pair(a, b, bins=bins)
            assert not out["status"].any() and out["power_a"].shape == (3, 2, C, n_bins)
            got = stacked(out).astype(ref.LD)
            want, bound = ref.pair_sums(a, b, table, n_bins, made), ref.forward_bound(a, b, table, n_bins, made)
            err = np.abs(got - want)
            frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)).astype(np.float64)
            for q, key in enumerate(ref.NAMES):
                worst[key] = max(worst[key], float(frac[..., q].max()))
            print(f"{H}x{W} C={C} {kind} {name}: error / bound " + " ".join(f"{key} {frac[..., q].max():.3g}"
                                                                            for q, key in enumerate(ref.NAMES)))
            assert (err <= bound).all(), f"{kind} {name}: worst error / bound {frac.max():.3g}"
            if kind == "offset" and name == "radial":
                # DC holds 1e4 times the power of the rest: what leaks from it is inside the bound of the other bins, and
                # that bound is far below them
                assert (bound[..., 1:, ref.PA] < 1e-6 * want[..., 1:, ref.PA])[want[..., 1:, ref.PA] > 0].all()
    print(f"{H}x{W} C={C}: worst error / bound " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_imaginary_cross_spectrum_cell_by_cell():
    """3 x 5 with one bin per coefficient: C_im is there, with the yardstick's sign, and conjugate cells carry opposite signs"""
    a, b = ref.pictures(5, (2, 3, 3, 3, 5), "gauss")
    table, n_bins = ref.cell_table(3, 5)
    got = stacked(pair(a, b, bins=table))[..., ref.CIM]
    want, bound = (f(a, b, table, n_bins)[..., ref.CIM] for f in (ref.pair_sums, ref.forward_bound))
    assert (np.abs(got - want) <= bound).all()
    clear = np.abs(want) > 1e6 * bound
    assert clear.sum() > 0.8 * clear.size and (got[clear] != 0).all() and (np.sign(got[clear]) == np.sign(want[clear])).all()
    cells = got.reshape(got.shape[:-1] + (3, 5))
    u, v = np.arange(3), np.arange(5)
    mirror = cells[..., (-u) % 3, :][..., (-v) % 5]
    assert np.array_equal(mirror[..., :, 1:], -cells[..., :, 1:])                  # v != 0: one is made from the other
    assert np.abs(mirror[..., :, 0] + cells[..., :, 0]).max() <= 2 * bound.max()   # v == 0: both are transformed
    assert (cells[..., 0, 0] == 0).all()                                           # DC of two real pictures


def test_power_entry_within_the_bound_and_on_flat_sets():
    a, b = ref.pictures(6, (5, 3, 28, 28), "gauss")
    table, cells = engine.radial_bins(28, 28)
    out = engine.device_spectrum(rows(a), 3, 28, 28)
    assert out["power"].shape == (5, 3, len(cells)) and out["status"].tolist() == [0] * 5
    want = ref.power_sums(a, table, len(cells))
    bound = ref.forward_bound(a, a, table, len(cells))[..., ref.PA]
    assert (np.abs(out["power"].cpu().numpy().astype(ref.LD) - want) <= bound).all()


# ------------------------------------------------------------------------------------------------ contracts
CONTRACT_SHAPES = [(3, 5, 3), (28, 28, 3), (64, 64, 1), (64, 7, 3), (1, 64, 1), (2, 2, 3)]


def contract_inputs(H, W, C, n=3, S=4):
    return ref.pictures(11 * H + W + C, (n, S, C, H, W), "gauss")


@pytest.mark.parametrize("H,W,C", CONTRACT_SHAPES)
def test_contract_1_rows_do_not_depend_on_their_surroundings(H, W, C):
    a, b = contract_inputs(H, W, C)
    n, S, E = 3, 4, C * H * W
    base = pair(a, b)
    A, B = rows(a), rows(b)
    for i, s in ((0, 0), (1, 2), (2, 3)):                                          # alone, as a flat set of one row
        one = engine.device_spectral_pair(A[i, s:s + 1], B[i, s:s + 1], C, H, W)
        assert all(same_bits(one[k][0], base[k][i, s]) for k in KEYS), f"row ({i}, {s}) alone"
    flat = engine.device_spectral_pair(A.reshape(n * S, E), B.reshape(n * S, E), C, H, W)
    assert all(same_bits(flat[k].reshape(base[k].shape), base[k]) for k in KEYS), "[Q, E]"
    # in a larger batch, at another position: state i -> 5 - 2 i, sample s -> 3 - s of a [6, 4] set of other rows
    fa, fb = ref.pictures(99, (6, 4, C, H, W), "offset")
    FA, FB = rows(fa), rows(fb)
    for i in range(n):
        FA[5 - 2 * i] = A[i].flip(0)
        FB[5 - 2 * i] = B[i].flip(0)
    big = engine.device_spectral_pair(FA, FB, C, H, W)
    assert all(same_bits(big[k][[5, 3, 1]].flip(1), base[k]) for k in KEYS), "larger batch, other position"
    # sample_grid-style views: every second state and a slice of the samples of a wider grid, 4 bytes off 16-byte alignment
    def grid_view(X, pad):
        buf = torch.full(((2 * n + 1) * (S + 3) * E + pad,), 7.0, device=DEV)[pad:].view(2 * n + 1, S + 3, E)
        view = buf[1::2, 2:2 + S]
        view.copy_(X)
        assert not view.is_contiguous()
        return view
    va, vb = grid_view(A, 1), grid_view(B, 3)
    viewed = engine.device_spectral_pair(va, vb, C, H, W)
    assert all(same_bits(viewed[k], base[k]) for k in KEYS), "strided views"
    need = _hip.load().dt_spectral_workspace_bytes(H, W, 1)
    roomy = engine.device_spectral_pair(A, B, C, H, W, workspace_bytes=need + 4096 + 16)
    assert all(same_bits(roomy[k], base[k]) for k in KEYS), "larger workspace"
    table, _ = engine.radial_bins(H, W)
    given = engine.device_spectral_pair(A, B, C, H, W, bins=dev(table))
    assert all(same_bits(given[k], base[k]) for k in KEYS), "the radial table passed in"
    with pytest.raises(ValueError):
        engine.device_spectral_pair(A, B, C, H, W, workspace_bytes=need - 1)


@pytest.mark.parametrize("H,W,C", CONTRACT_SHAPES)
def test_contracts_2_to_5(H, W, C):
    a, b = contract_inputs(H, W, C)
    holes, _ = ref.holes_table(H, W)
    for bins in (None, holes):
        base = pair(a, b, bins=bins)
        power = engine.device_spectrum(rows(a), C, H, W, bins=bins)
        assert same_bits(power["power"], base["power_a"]), "2: the power entry has the bits of the pair's P_a"
        swapped = pair(b, a, bins=bins)
        assert same_bits(swapped["power_a"], base["power_b"]) and same_bits(swapped["power_b"], base["power_a"]), "3: swap"
        assert same_bits(swapped["error"], base["error"]) and same_bits(swapped["cross"][..., 0], base["cross"][..., 0]), "3: swap"
        assert torch.equal(swapped["cross"][..., 1], -base["cross"][..., 1]), "3: C_im is negated"
        if bins is not None and H * W > 4:              # (in a table that is symmetric under (u, v) -> (-u, -v) C_im cancels)
            assert (base["cross"][..., 1] != 0).any()
        copied = engine.device_spectral_pair(rows(a), rows(a).clone(), C, H, W, bins=bins)
        assert (copied["error"] == 0).all() and (copied["cross"][..., 1] == 0).all(), "4: D and C_im of a copy are exactly 0"
        assert same_bits(copied["power_a"], base["power_a"]) and same_bits(copied["power_b"], base["power_a"]), "4: copy"
        assert same_bits(copied["cross"][..., 0], base["power_a"]), "4: C_re of a copy has the bits of P_a"
        for k in (-3, 5):
            scaled = pair(a * np.float32(2.0 ** k), b * np.float32(2.0 ** k), bins=bins)
            assert all(same_bits(scaled[key], base[key] * 4.0 ** k) for key in KEYS), f"5: scaling by 2^{k}"


# ------------------------------------------------------------------------------------------------ non-finite rows, sample sums
@pytest.mark.parametrize("H,W,C", [(16, 16, 3), (3, 5, 1), (64, 64, 1)])
def test_nonfinite_rows_and_sample_sums(H, W, C):
    a, b = contract_inputs(H, W, C, n=4, S=5)
    clean = pair(a, b)
    summed = pair(a, b, sum_samples=True)
    assert summed["count"].tolist() == [5] * 4 and torch.equal(summed["status"], clean["status"])
    for key in KEYS:                                                            # the rows added in index order, in float64
        per_row = clean[key].cpu().numpy()
        acc = np.zeros_like(per_row[:, 0])
        for s in range(5):
            acc = acc + per_row[:, s]
        assert same_bits(summed[key], acc), key
    a2, b2 = a.copy(), b.copy()
    a2[1, 2, C - 1, H - 1, W // 2] = np.nan
    b2[3, 0, 0, 0, 0] = -np.inf
    out = pair(a2, b2)
    flagged = np.zeros((4, 5), dtype=bool)
    flagged[1, 2] = flagged[3, 0] = True
    assert np.array_equal(out["status"].cpu().numpy(), flagged.astype(np.int32))
    for key in KEYS:
        got = out[key].cpu().numpy()
        assert np.isnan(got[flagged]).all() and same_bits(got[~flagged], clean[key].cpu().numpy()[~flagged]), key
    power = engine.device_spectrum(rows(b2), C, H, W)
    assert power["status"].sum().item() == 1 and power["status"][3, 0] == 1 and torch.isnan(power["power"][3, 0]).all()
    summed = pair(a2, b2, sum_samples=True)
    assert summed["count"].tolist() == [5, 4, 5, 4]
    for key in KEYS:
        per_row = clean[key].cpu().numpy()
        acc = np.zeros_like(per_row[:, 0])
        for s in range(5):
            acc = acc + np.where(flagged[:, s].reshape((4,) + (1,) * (acc.ndim - 1)), 0.0, per_row[:, s])
        got = summed[key].cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got, acc), key
    one = engine.device_spectrum(rows(a2), C, H, W, sum_samples=True)
    assert one["count"].tolist() == [5, 4, 5, 5] and one["power"].shape == clean["power_a"][:, 0].shape
    flat = engine.device_spectrum(rows(a2).reshape(20, -1), C, H, W, sum_samples=True)
    assert flat["count"].item() == 19 and flat["power"].shape == clean["power_a"].shape[2:]


# ------------------------------------------------------------------------------------------------ Parseval
@pytest.mark.parametrize("H,W,C", [(16, 16, 3), (28, 28, 1), (64, 64, 1), (3, 5, 3)])
def test_parseval_against_the_pair_metric_kernel(H, W, C):
    """sum over bins and channels of D / (H W) is the squared error of the two rows: fp32 inputs, fp64 sums on both sides"""
    a, b = contract_inputs(H, W, C)
    out = pair(a, b)
    got = out["error"].sum(dim=(-2, -1)).cpu().numpy() / (H * W)                    # [n, S]
    sums, _ = engine.device_pair_metrics(rows(a), rows(b))
    want = sums[:, :, 0].cpu().numpy().T                                           # [S, n] -> [n, S]
    rel = np.abs(got - want) / want
    print(f"{H}x{W} C={C}: Parseval, worst relative difference {rel.max():.3g}")
    assert (rel <= 1e-6).all()


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
    return cfg, teacher, student, grids


def test_spectral_pairs_against_the_yardstick(models):
    """3 states, 4 samples, 16 x 16: the derived band metrics equal the yardstick's to 1e-12"""
    cfg, teacher, student, (X, Y) = trajectory_pair(models)
    assert X.shape == (3, 4, 768)
    res = spectral.spectral_pairs(X, Y, 3, 16, 16)
    table, cells = engine.radial_bins(16, 16)
    a, b = (t.cpu().numpy().reshape(3, 4, 3, 16, 16) for t in (X, Y))
    sums = ref.pair_sums(a, b, table, len(cells)).sum(axis=(1, 2))                  # samples and channels: [3, bins, 5]
    want = spectral.derived_metrics(sums[..., ref.PA], sums[..., ref.PB], sums[..., ref.CRE], sums[..., ref.D],
                                    np.full(3, 4), cells, 3, 16, 16)
    assert res["count"].tolist() == [4, 4, 4] and not res["status"].any() and res["status"].shape == (3, 4)
    assert res["radius"].tolist() == list(range(len(cells))) and np.array_equal(res["cells_per_bin"], cells)
    for key in ("power_teacher", "power_student", "band_correlation", "relative_error", "log_spectral_distance"):
        w = want[key].astype(np.float64)
        assert res[key].shape == w.shape and np.isfinite(w).all(), key
        assert (np.abs(res[key] - w) <= 1e-12 * np.maximum(np.abs(w), 1e-300)).all(), key
    assert (res["relative_error"][0] == 0).all() and (res["band_correlation"][0] == 1).all()     # the shared start noise
    assert (res["relative_error"][1:] > 0).all()
    lists = [[x.reshape(4, 3, 16, 16).cpu() for x in X], [(y.reshape(4, 3, 16, 16), 2 - i) for i, y in enumerate(Y)]]
    again = spectral.spectral_trajectories(*lists)
    for key in res:
        assert np.array_equal(again[key], res[key], equal_nan=True), key
    with pytest.raises(ValueError):
        spectral.spectral_trajectories(lists[0], lists[1][:2])


def test_spectral_sweep_tiny(models, tmp_path):
    cfg, teacher, student, _ = trajectory_pair(models)
    twin = copy.deepcopy(teacher)
    scales = [None, 3.0]
    res = spectral.spectral_sweep(teacher, [twin, student], cfg, scales, 4, output_dir=str(tmp_path))
    n_bins = len(engine.radial_bins(16, 16)[1])
    for key in ("power_teacher", "power_student", "band_correlation", "relative_error"):
        assert res[key].shape == (2, 2, 3, n_bins), key
    assert res["log_spectral_distance"].shape == res["count"].shape == (2, 2, 3) and (res["count"] == 4).all()
    assert res["status"].shape == (2, 2, 3, 4) and not res["status"].any() and res["states"].tolist() == [0, 1, 2]
    assert np.isnan(res["guidance_scales"][0]) and res["guidance_scales"][1] == 3.0
    has = res["power_teacher"][0] > 0
    assert has.all()
    assert (res["relative_error"][0] == 0).all() and (res["band_correlation"][0] == 1).all()   # a student that is the teacher
    assert (res["log_spectral_distance"][0] == 0).all()
    assert (res["relative_error"][1][:, 1:] > 0).all() and np.isfinite(res["band_correlation"][1]).all()
    assert not np.array_equal(res["relative_error"][1][0], res["relative_error"][1][1])        # the scales differ
    for k in range(2):
        with np.load(os.path.join(str(tmp_path), f"spectral_student_{k}.npz")) as f:
            assert sorted(f.files) == sorted(res)
            assert np.array_equal(f["relative_error"], res["relative_error"][k]) and f["status"].shape == (2, 3, 4)
            assert np.array_equal(f["radius"], np.arange(n_bins)) and f["states"].tolist() == [0, 1, 2]
    # one cell run alone: (student 1, scale 3.0)
    from distillation_trajectories_amd.analysis.trajectory_engine import sample_grid
    from distillation_trajectories_amd.synthetic import noise_table
    table = noise_table(42, 4 + 2 - 1, (1, 3, 16, 16)).reshape(5, -1).to(DEV)
    X, Y = (sample_grid(engine.UNetHandle.for_module(m), table, 0, 4, 2, [3.0], 16, 16)[3.0] for m in (teacher, student))
    alone = spectral.spectral_pairs(X, Y, 3, 16, 16)
    for key in ("power_teacher", "power_student", "band_correlation", "relative_error", "log_spectral_distance", "count", "status"):
        assert np.array_equal(alone[key], res[key][1][1]), key
    every = spectral.spectral_sweep(teacher, [student], cfg, [3.0], 4, every=2, output_dir=str(tmp_path / "every"))
    assert every["states"].tolist() == [0, 2] and np.array_equal(every["relative_error"][0][0], res["relative_error"][1][1][[0, 2]])
