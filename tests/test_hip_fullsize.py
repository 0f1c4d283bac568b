"""GPU checks at BASELINE.json's full sizes, through size-independent properties plus oracle spot checks.

configs[1]: teacher vs sf=0.5, 16x16, T=50, batch 256, p_sample_loop CFG.
configs[4]: 32x32 (CIFAR shape), teacher, CFG 7 -- forward parity and a short loop.
configs[2]/[3]: size sweep x CFG grid through grid.grid_metrics on one rank.
"""
import copy
import os

import numpy as np
import pytest
import torch

import metrics_ref64 as ref64
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.config import Config
from distillation_trajectories_amd.models import DiffusionUNet
from distillation_trajectories_amd.synthetic import make_model
from oracle import metrics_ref, sampler_ref, unet_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _loop(h, x_T, z, idx, coef, w, B, E, H):
    from distillation_trajectories_amd._hip import COND_NONE, COND_ONE, RULE_PSAMPLE
    n = len(idx)
    traj = torch.empty(n + 1, B, E, device=DEV)
    traj[0].copy_(x_T)
    has_noise = [i > 0 for i in idx]
    shift, k = [], 0
    for f in has_noise:
        shift.append(k * B)
        k += int(f)
    tb = h.time_bias([i for i in idx for _ in (0, 1)], [COND_NONE, COND_ONE] * n)
    h.sample(RULE_PSAMPLE, traj, H, H, tb, 2, coef, has_noise, z=z, z_shift=shift, w_scalar=w)
    return traj


@pytest.fixture(scope="module")
def bench_pair(models):
    return [copy.deepcopy(models(sf)).to(DEV) for sf in (1.0, 0.5)]


def test_config1_full_batch_loop_properties(bench_pair, models):
    """B=256, T=50, two passes per step: permutation equivariance of whole trajectories (bit-exact) and
    the first steps of four samples against the CPU oracle."""
    from distillation_trajectories_amd.utils.diffusion import get_diffusion_params, psample_coefficients, timestep_indices
    B, T, H, E = 256, 50, 16, 768
    idx = timestep_indices(T, T)
    coef = psample_coefficients(get_diffusion_params(T), idx)
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn(B, E, generator=g)
    z = torch.randn((T - 1) * B, E, generator=g)
    perm = torch.randperm(B, generator=g)
    for m, sf in zip(bench_pair, (1.0, 0.5)):
        h = engine.UNetHandle.for_module(m)
        traj = _loop(h, x_T.to(DEV), z.to(DEV), idx, coef, 1.0, B, E, H)
        assert torch.isfinite(traj).all()
        zp = z.reshape(T - 1, B, E)[:, perm].reshape(-1, E).contiguous()
        traj_p = _loop(h, x_T[perm].to(DEV), zp.to(DEV), idx, coef, 1.0, B, E, H)
        assert torch.equal(traj_p, traj[:, perm.to(DEV)]), f"sf={sf}: rows of the batch must be independent"
        # oracle: 3 steps of samples 0..3
        sd = models(sf).state_dict()
        fn = lambda x, t, c: unet_ref.unet_forward(sd, x, t, c)    # noqa: E731
        params = sampler_ref.diffusion_params(T)
        x = x_T[:4].reshape(4, 3, H, H)
        with torch.no_grad():
            for s, i in enumerate(idx[:3]):
                x = sampler_ref.p_sample(fn, x, torch.full((4,), i, dtype=torch.long), i, params, 1.0,
                                         noise=z.reshape(T - 1, B, E)[s, :4].reshape(4, 3, H, H))
                got = traj[s + 1, :4].cpu().reshape(4, 3, H, H)
                assert torch.allclose(got, x, rtol=1e-4, atol=1e-4), (sf, s, (got - x).abs().max())


def test_config1_full_batch_metrics(bench_pair):
    """256 pairs x 51 states through the metric kernels: oracle spot checks + structural properties."""
    g = torch.Generator().manual_seed(6)
    n, B, E = 51, 256, 768
    X = torch.randn(n, B, E, generator=g).cumsum(0) * 0.05
    Y = X + 0.02 * torch.randn(n, B, E, generator=g)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    sums = engine.device_metric_sums(Xd, Yd).cpu().numpy()
    w1 = engine.device_wasserstein(Xd, Yd).cpu().numpy()
    swapped = engine.device_metric_sums(Yd, Xd).cpu().numpy()
    assert np.array_equal(swapped[..., 0], sums[..., 0]) and np.array_equal(swapped[..., 1], sums[..., 2])
    same = engine.device_metric_sums(Xd, Xd).cpu().numpy()
    assert not same[..., 0].any() and np.array_equal(same[..., 1], same[..., 2]) and not same[:, 0, 3].any()
    assert not engine.device_wasserstein(Xd, Xd).cpu().numpy().any()
    vec = engine.batch_scalar_metrics(sums, w1, 256, E)
    for b in (0, 97, 255):
        a = [X[i, b].reshape(1, 3, 16, 16) for i in range(n)]
        c = [Y[i, b].reshape(1, 3, 16, 16) for i in range(n)]
        want = metrics_ref.compute_trajectory_metrics(a, c)
        for k in engine.SCALAR_KEYS:
            if k == "trajectory_mse":
                continue
            assert abs(vec[k][b] - float(want[k])) <= 1e-5 * max(abs(float(want[k])), 1e-9), (b, k)


def test_config4_cifar_shape_forward_and_loop(models):
    """32x32x3, teacher, CFG w=7: forward vs oracle at B=2 and a 4-step loop at B=128 (finite, row-independent)."""
    from distillation_trajectories_amd.utils.diffusion import get_diffusion_params, psample_coefficients, timestep_indices
    m = copy.deepcopy(models(1.0)).to(DEV)
    sd = models(1.0).state_dict()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 32, 32, generator=g)
    t = torch.tensor([999, 999])
    with torch.no_grad():
        want = unet_ref.unet_forward(sd, x, t, torch.ones(2, 1))
    got = m(x.to(DEV), t.to(DEV), torch.ones(2, 1, device=DEV))
    assert torch.allclose(got.cpu(), want, rtol=1e-4, atol=2e-5), (got.cpu() - want).abs().max()
    B, H, E, T = 128, 32, 3072, 1000
    idx = timestep_indices(T, T)[:4]
    coef = psample_coefficients(get_diffusion_params(T), idx)
    x_T = torch.randn(B, E, generator=g)
    z = torch.randn(4 * B, E, generator=g)
    h = engine.UNetHandle.for_module(m)
    traj = _loop(h, x_T.to(DEV), z.to(DEV), idx, coef, 7.0, B, E, H)
    assert torch.isfinite(traj).all()
    fn = lambda a, b, c: unet_ref.unet_forward(sd, a, b, c)    # noqa: E731
    with torch.no_grad():
        ref = sampler_ref.p_sample(fn, x_T[:2].reshape(2, 3, H, H), torch.full((2,), idx[0], dtype=torch.long), idx[0],
                                   sampler_ref.diffusion_params(T), 7.0, noise=z[:2].reshape(2, 3, H, H))
    assert torch.allclose(traj[1, :2].cpu().reshape(2, 3, H, H), ref, rtol=1e-4, atol=1e-4)


def test_config3_grid_one_rank_matches_compare_trajectories(models):
    """Size sweep x CFG grid through grid_metrics equals per-student compare_trajectories calls."""
    from distillation_trajectories_amd.analysis.trajectory_engine import compare_trajectories
    from distillation_trajectories_amd.grid import grid_metrics
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 12
    teacher = copy.deepcopy(models(0.5)).to(DEV)
    students = [copy.deepcopy(models(sf)).to(DEV) for sf in (0.01, 0.2)]
    scales = [1.0, 3.0, 20.0]
    grid = grid_metrics(teacher, students, cfg, scales, num_samples=6, rank=0, world=1)
    for i, s in enumerate(students):
        res = compare_trajectories(teacher, s, cfg, guidance_scales=scales, num_samples=6)["student_metrics"]
        for gs in scales:
            for k, v in res[gs].items():
                a, b = grid[i][gs][k], v
                assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-9 * max(abs(b), 1e-12), (i, gs, k, a, b)


def test_grid_32x32_subsampled_wasserstein_matches_compare_trajectories(models):
    """E = 3072 > 1000: the Wasserstein term samples 1000 coordinates per step from per-sample tables (legacy MT19937, seeded
    by the sample seed); in the grid one table row serves every row block of a mixed batch (index_row repeated per block).
    A small 32 x 32 grid (2 samples, T = 6, one single-pass and two CFG scales) against compare_trajectories."""
    from distillation_trajectories_amd.analysis.trajectory_engine import compare_trajectories
    from distillation_trajectories_amd.grid import grid_metrics
    cfg = Config()
    cfg.image_size, cfg.timesteps = 32, 6
    teacher = copy.deepcopy(models(0.2)).to(DEV)
    students = [copy.deepcopy(models(0.01)).to(DEV)]
    scales = [1.0, 3.0, 7.0]
    grid = grid_metrics(teacher, students, cfg, scales, num_samples=2, rank=0, world=1)
    res = compare_trajectories(teacher, students[0], cfg, guidance_scales=scales, num_samples=2)["student_metrics"]
    for gs in scales:
        for k, v in res[gs].items():
            a = grid[0][gs][k]
            assert (np.isnan(a) and np.isnan(v)) or abs(a - v) <= 1e-9 * max(abs(v), 1e-12), (gs, k, a, v)
    assert res[3.0]["mean_wasserstein"] > 0


# ------------------------------------------------------------------ round 2: parity at the benchmark's own model sizes
def _close(got, want, rtol, atol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    tol = atol + rtol * np.abs(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.all(err <= tol), f"{what}: max err {err.max():.3e} at tol {tol.flat[err.argmax()]:.3e} (max |want| {np.abs(want).max():.3e})"


def _check_metric_dict(got, want, rel, what):
    """Reference metric dict (json) vs ours: scalars and per-step lists within ``rel``, identical NaN positions,
    trajectory_mse on its pre-transform quantity 1000 * mean step-MSE = 1 - expm1(value)."""
    assert set(got) == set(want), what
    for k, w in want.items():
        g = got[k]
        if isinstance(w, list):
            assert len(g) == len(w), (what, k)
            _close(g, w, rel, 1e-7, f"{what} {k}")
        elif isinstance(w, float) and np.isnan(w):
            assert np.isnan(float(g)), (what, k)
        elif k == "trajectory_mse":
            _close(1.0 - np.expm1(float(g)), 1.0 - np.expm1(float(w)), rel, 1e-9, f"{what} {k} (pre-transform)")
        else:
            _close(float(g), float(w), rel, 1e-9, f"{what} {k}")


def test_pair3_real_size_trajectories_and_metrics(golden, models):
    """Teacher sf=1.0 vs student sf=0.5, gs=3, seed 46, T=50 (reference analysis/trajectory_engine.py:24-115): the
    HIP loop's 51 states against the reference's, then the metrics of the HIP trajectories against pair3.metrics."""
    from distillation_trajectories_amd.analysis.metrics.trajectory_metrics import compute_trajectory_metrics
    from distillation_trajectories_amd.analysis.trajectory_engine import generate_trajectory
    from distillation_trajectories_amd.synthetic import seeded_noise
    arrays, meta = golden
    c = next(m for m in meta["metric_cases"] if m["key"] == "pair3")
    assert (c["teacher_sf"], c["student_sf"], c["gs"], c["seed"], c["T"]) == (1.0, 0.5, 3.0, 46, 50)
    noise = seeded_noise(c["seed"], (1, 3, 16, 16))
    trajs = {}
    for who, sf in (("teacher", 1.0), ("student", 0.5)):
        m = copy.deepcopy(models(sf)).to(DEV)
        tr = generate_trajectory(m, noise, c["T"], torch.device(DEV), seed=c["seed"], guidance_scale=c["gs"])
        want = arrays[f"pair3_{who}"]
        got = torch.stack(tr).numpy()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[-1], got[-2])
        # error growth over the 50 dependent steps: reported per step against the state's own scale
        rel = np.abs(got - want).reshape(len(want), -1).max(1) / np.abs(want).reshape(len(want), -1).max(1)
        print(f"pair3 {who}: max |err| / max |state| per step: first {rel[1]:.2e}, mid {rel[25]:.2e}, last {rel[-1]:.2e}")
        _close(got, want, 1e-4, 1e-4 * float(np.abs(want).max()), f"pair3 {who} trajectory")
        trajs[who] = tr
    _check_metric_dict(compute_trajectory_metrics(trajs["teacher"], trajs["student"]), c["metrics"], 1e-4, "pair3")


def test_r02_forward_all_size_factors_golden(golden_r02, models):
    """Every size factor of configs[2] the first fixture file lacks (channels 16 ... 230, models.py:101-110)."""
    arrays, meta = golden_r02
    seen = set()
    for c in meta["forward_cases"]:
        m = copy.deepcopy(models(c["sf"])).to(DEV)
        x = seeded_noise_(c["seed"], (c["b"], 3, c["h"], c["h"]))
        t = torch.full((c["b"],), c["t"], dtype=torch.long)
        cond = None if c["cond"] == "none" else torch.full((c["b"], 1), 0.0 if c["cond"] == "zero" else 1.0)
        y = m(x.to(DEV), t.to(DEV), None if cond is None else cond.to(DEV))
        _close(y.cpu().numpy(), arrays[c["key"]], 1e-4, 2e-5, str(c))
        seen.add(c["sf"])
    assert seen == {0.05, 0.1, 0.3, 0.4, 0.6, 0.7, 0.75, 0.8, 0.9}


def seeded_noise_(seed, shape):
    from distillation_trajectories_amd.synthetic import seeded_noise
    return seeded_noise(seed, shape)


def test_r02_config0_teacher_loop_golden(golden_r02, models):
    """configs[0]: teacher p_sample_loop, B=8, T=50 against the reference's whole trajectory."""
    from distillation_trajectories_amd.utils.diffusion import get_diffusion_params, p_sample_loop
    arrays, meta = golden_r02
    c = meta["config0_case"]
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, c["timesteps"]
    m = copy.deepcopy(models(c["sf"])).to(DEV)
    torch.manual_seed(c["global_seed"])
    img, tr = p_sample_loop(m, (c["b"], 3, 16, 16), c["sample_steps"], get_diffusion_params(c["sample_steps"], cfg),
                            device=torch.device(DEV), config=cfg, track_trajectory=True, guidance_scale=c["w"])
    got, want = torch.stack(tr).numpy(), arrays[c["key"]]
    rel = np.abs(got - want).reshape(len(want), -1).max(1) / np.abs(want).reshape(len(want), -1).max(1)
    print(f"config0 teacher: max |err| / max |state| per step: first {rel[1]:.2e}, mid {rel[25]:.2e}, last {rel[-1]:.2e}")
    _close(got, want, 1e-4, 1e-4 * float(np.abs(want).max()), "configs[0] teacher trajectory")


def test_r02_config4_tail_golden(golden_r02, models):
    """configs[4]: 32x32, T=1000, w=7.  The random-init teacher is unstable under w=7 (states reach 3e9 in the
    reference too), so the comparison is made where it is meaningful: (a) every one of the last 50 steps restarted
    from the reference's own state (50 different (t, state) pairs through U-Net + CFG mix + update), (b) the
    free-running 50-step tail from the reference's state after 950 steps."""
    from distillation_trajectories_amd._hip import RULE_PSAMPLE
    from distillation_trajectories_amd.utils.diffusion import get_diffusion_params, psample_coefficients, timestep_indices
    arrays, meta = golden_r02
    c = meta["config4_case"]
    tail = arrays[c["key"]]
    B, H, E, T, first = c["b"], c["h"], 3 * c["h"] * c["h"], c["sample_steps"], c["first_entry"]
    shape = (B, 3, H, H)
    torch.manual_seed(c["global_seed"])
    torch.randn(shape)
    zs = torch.stack([torch.randn(shape) for _ in range(T - 1)]).reshape(T - 1, B, E)
    idx = timestep_indices(T, c["timesteps"])
    cfg = Config()
    cfg.image_size, cfg.timesteps = H, c["timesteps"]
    coef = psample_coefficients(get_diffusion_params(T, cfg), idx)
    h = engine.UNetHandle.for_module(copy.deepcopy(models(c["sf"])).to(DEV))
    n = T - first
    # (a) teacher-forced single steps
    worst = 0.0
    for k in range(first, T):
        tr = _loop_from(h, torch.from_numpy(tail[k - first]).reshape(B, E), zs[k:k + 1] if idx[k] > 0 else None, [idx[k]], [coef[k]],
                        c["w"], B, E, H)
        got, want = tr[1].cpu().numpy().reshape(shape), tail[k - first + 1]
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
        _close(got, want, 1e-4, 1e-4 * float(np.abs(want).max()), f"configs[4] single step {k} (t={idx[k]})")
    # (b) free-running tail
    tr = _loop_from(h, torch.from_numpy(tail[0]).reshape(B, E), zs[first:], idx[first:], coef[first:], c["w"], B, E, H)
    got = tr.cpu().numpy().reshape(n + 1, *shape)
    rel = np.abs(got - tail).reshape(n + 1, -1).max(1) / np.abs(tail).reshape(n + 1, -1).max(1)
    print(f"configs[4]: single-step worst {worst:.2e}; free-running tail max |err| / max |state|: step 1 {rel[1]:.2e}, "
          f"25 {rel[25]:.2e}, 50 {rel[-1]:.2e}")
    assert np.isfinite(got).all()
    assert rel.max() < 5e-3, rel      # an unstable map amplifies fp32 re-association noise; (a) is the parity check


def _loop_from(h, x0, z, idx, coef, w, B, E, H):
    from distillation_trajectories_amd._hip import COND_NONE, COND_ONE, RULE_PSAMPLE
    n = len(idx)
    traj = torch.empty(n + 1, B, E, device=DEV)
    traj[0].copy_(x0)
    has_noise = [i > 0 for i in idx]
    shift, k = [], 0
    for f in has_noise:
        shift.append(k * B)
        k += int(f)
    zd = z.reshape(-1, E).to(DEV) if z is not None and len(z) else None
    tb = h.time_bias([i for i in idx for _ in (0, 1)], [COND_NONE, COND_ONE] * n)
    h.sample(RULE_PSAMPLE, traj, H, H, tb, 2, coef, has_noise, z=zd, z_shift=shift, w_scalar=w)
    return traj


def test_config2_full_size_sweep_grid(golden_r02, models):
    """configs[2]: all 11 size factors x CFG {1,3,7,20} through grid_metrics (2 samples, T=50); the (0.6, 0.9) x (1, 7)
    cells against the reference's compare_trajectories (scripts/analysis/analyze_trajectory_metrics.py:476-505)."""
    from distillation_trajectories_amd.grid import grid_metrics
    from distillation_trajectories_amd.utils.metric_transformations import transform_metrics
    _, meta = golden_r02
    sizes = [0.01, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]
    scales = [1.0, 3.0, 7.0, 20.0]
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 50
    teacher = copy.deepcopy(models(1.0)).to(DEV)
    students = [copy.deepcopy(models(sf)).to(DEV) for sf in sizes]
    grid = grid_metrics(teacher, students, cfg, scales, num_samples=2, rank=0, world=1)
    assert len(grid) == len(sizes)
    for i, sf in enumerate(sizes):
        for gs in scales:
            cell = grid[i][gs]
            assert set(cell) == set(engine.SCALAR_KEYS)
            for k, v in cell.items():
                assert np.isfinite(v) or k == "trajectory_mse", (sf, gs, k, v)
            t = transform_metrics(cell["path_length_similarity"], cell["trajectory_mse"], cell["mean_directional_consistency"],
                                  cell["distribution_similarity"])
            assert all(0.0 <= float(t[k]) <= 1.0 or np.isnan(t[k]) for k in ("trajectory_mse", "distribution_similarity"))
    # the sf = 1.0 "student" has the teacher's weights: the same trajectories up to the two handles' own launch plans
    for gs in scales:
        assert grid[-1][gs]["endpoint_distance"] < 1e-3 and grid[-1][gs]["mean_wasserstein"] < 1e-5, grid[-1][gs]
    for c in meta["grid_cells"]:
        i = sizes.index(c["student_sf"])
        for gs in c["guidance_scales"]:
            want = c["result"]["student_metrics"][str(gs)]
            got = {k: grid[i][gs][k] for k in want}
            assert set(want) == set(engine.SCALAR_KEYS) - {"path_alignment"}     # np.float32 in the reference: not averaged (:171-175)
            _check_metric_dict(got, want, 1e-4, f"grid cell sf={c['student_sf']} gs={gs}")


def test_forward_64x64_autotuned(models, monkeypatch):
    """64-pixel rows: the strip kernel cannot stage W + 1 = 65 halo pixels at the top level, so the autotuner must
    fall back to the plain kernel there instead of failing (batch 4 x 64 x 64 = 16384 rows is where opt-in tuning starts)."""
    monkeypatch.setenv("DT_AUTOTUNE", "1")
    for sf in (0.2, 1.0):
        m = copy.deepcopy(models(sf)).to(DEV)
        sd = models(sf).state_dict()
        g = torch.Generator().manual_seed(64)
        x = torch.randn(4, 3, 64, 64, generator=g)
        t = torch.full((4,), 31, dtype=torch.long)
        with torch.no_grad():
            want = unet_ref.unet_forward(sd, x, t, torch.ones(4, 1))
        got = m(x.to(DEV), t.to(DEV), torch.ones(4, 1, device=DEV))
        h = engine.UNetHandle.for_module(m)
        assert (4, 64, 64) in h._tuned
        kinds = {(c[0], c[1]): c[5] for c in h.conv_choices(4, 64, 64)}
        assert "strip" not in kinds[("enc1", "conv2")], kinds
        _close(got.cpu().numpy(), want.numpy(), 1e-4, 2e-5, f"64x64 sf={sf}")


def test_unchanged_caller_flow_with_aliases(models, tmp_path, monkeypatch):
    """The flow of scripts/analysis/analyze_trajectory_metrics.py:458-505 with its OWN import lines (:22-26), made to
    resolve to this package by install_aliases(): state_dict checkpoints on disk -> load_state_dict -> eval / to(device)
    -> compare_trajectories per size factor -> transform_metrics per heat-map cell (:95-100)."""
    import distillation_trajectories_amd as pkg
    monkeypatch.chdir(tmp_path)
    names = pkg.install_aliases()
    try:
        assert "config.config" in names and "analysis.trajectory_engine" in names
        from config.config import Config as RefConfig                                # noqa: the reference's import lines
        from models import DiffusionUNet as RefUNet
        from analysis.trajectory_engine import compare_trajectories
        from analysis.metrics.trajectory_metrics import compute_trajectory_metrics    # noqa: F401
        from utils.metric_transformations import transform_metrics
        config = RefConfig()
        config.timesteps = 6
        config.image_size = 16
        # checkpoints as the training scripts leave them (scripts/train_teacher.py:86, train_students.py:185-187)
        os.makedirs(config.teacher_models_dir)
        torch.save(models(1.0).state_dict(), os.path.join(config.teacher_models_dir, "model_epoch_200.pt"))
        size_factors = [0.2, 0.5]
        for sf in size_factors:
            d = os.path.join(config.student_models_dir, f"size_{sf}")
            os.makedirs(d)
            torch.save(models(0.01).state_dict(), os.path.join(d, "model_epoch_3.pt"))       # stale, wrong-size: never loaded
            torch.save(models(sf).state_dict(), os.path.join(d, "model_epoch_12.pt"))   # "latest" = highest epoch
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        teacher_model = RefUNet(config, size_factor=1.0)
        teacher_model.load_state_dict(torch.load(os.path.join(config.teacher_models_dir, "model_epoch_200.pt"), map_location=device))
        teacher_model.eval()
        teacher_model = teacher_model.to(device)
        guidance_scales = [1.0, 3.0]
        metrics_by_size = {}
        for size_factor in size_factors:
            size_dir = os.path.join(config.student_models_dir, f"size_{size_factor}")
            model_files = [f for f in os.listdir(size_dir) if f.startswith("model_epoch_") and f.endswith(".pt")]
            latest_model = max(model_files, key=lambda x: int(x.split("_")[2].split(".")[0]))
            assert latest_model == "model_epoch_12.pt"
            student_model = RefUNet(config, size_factor=size_factor)
            student_model.load_state_dict(torch.load(os.path.join(size_dir, latest_model), map_location=device))
            student_model = student_model.to(device)
            student_model.eval()
            metrics_by_size[size_factor] = compare_trajectories(teacher_model, student_model, config, guidance_scales=guidance_scales,
                                                                size_factor=size_factor, num_samples=2)
        # oracle on the same checkpoints
        t_sd = models(1.0).state_dict()
        for sf in size_factors:
            s_sd = models(sf).state_dict()
            with torch.no_grad():
                ref = sampler_ref.compare_trajectories(lambda x, t, c: unet_ref.unet_forward(t_sd, x, t, c),
                                                       lambda x, t, c, s_sd=s_sd: unet_ref.unet_forward(s_sd, x, t, c),
                                                       config, guidance_scales=guidance_scales, num_samples=2)
            for gs in guidance_scales:
                got, want = metrics_by_size[sf]["student_metrics"][gs], ref["student_metrics"][gs]
                _check_metric_dict({k: got[k] for k in want}, {k: float(v) for k, v in want.items()}, 1e-4, f"caller flow sf={sf} gs={gs}")
                cell = transform_metrics(got["path_length_similarity"], got["trajectory_mse"], got["mean_directional_consistency"],
                                         got["distribution_similarity"])
                assert set(cell) == {"path_length_similarity", "trajectory_mse", "mean_directional_consistency", "distribution_similarity"}
    finally:
        pkg.remove_aliases()


def test_two_ranks_shard_the_grid_like_one(tmp_path):
    """configs[3] in miniature on one GPU: bench.py's own launcher starts 2 ranks (gloo stands in for RCCL so that both
    can share this GPU), each runs its sample shard of the 11-size x 4-scale grid on the HIP path, the metric rows are
    all-gathered, and the gathered cells must equal those of ONE rank running all the samples."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DT_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)

    def run(gpus, batch):
        res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", "2", "--gpus", str(gpus), "--batch", str(batch),
                              "--steps", "1", "--warmup", "0", "--no-profile", "--no-cpu-baseline",
                              "--dump-outputs", str(tmp_path / f"dump{gpus}")], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    two, one = run(2, 3), run(1, 6)
    # rank 0 dumps every rank's cells after the all-gather: all finite, the same set of arrays as one rank's
    assert sorted(os.listdir(tmp_path / "dump2")) == sorted(os.listdir(tmp_path / "dump1")) and os.listdir(tmp_path / "dump1")
    for f in os.listdir(tmp_path / "dump1"):
        for d in ("dump1", "dump2"):
            a = np.load(tmp_path / d / f)
            assert a.shape == (11, 4, 6) and np.all(np.isfinite(a)), (d, f)
    assert two["n_gpus"] == 2 and [r["rank"] for r in two["ranks"]] == [0, 1] and one["n_gpus"] == 1
    assert two["metric_check"]["cells"] == one["metric_check"]["cells"] == 11 * 4 * 6
    a, b = two["metric_check"]["path_length_similarity_sf0.5_gs3"], one["metric_check"]["path_length_similarity_sf0.5_gs3"]
    assert abs(a - b) <= 1e-6 * abs(b), (a, b)


@pytest.mark.parametrize("shape", [(51, 256, 768), (7, 5, 1024), (4, 3, 1540), (3, 2, 3072), (2, 1, 4096), (5, 4, 12)])
def test_one_pass_pair_metrics_match_the_two_kernels(shape):
    """dt_traj_pair_metrics (sums + register / cross-lane bitonic sort in one launch) against dt_traj_metrics and
    dt_traj_wasserstein (LDS sort): the sorted order statistics are the same numbers, so W1 agrees to float64 summation
    order; E = 768 is every 16x16x3 configuration, 1540 / 3072 / 4096 exercise 8 and 16 coordinates per thread and the +inf
    padding, 12 a nearly empty workgroup."""
    n, B, E = shape
    g = torch.Generator().manual_seed(n * 1000 + E)
    X = (torch.randn(n, B, E, generator=g).cumsum(0) * 0.05).to(DEV)
    Y = (X.cpu() + 0.02 * torch.randn(n, B, E, generator=g)).to(DEV)
    sums, w1 = engine.device_pair_metrics(X, Y)
    ref_s, ref_w = engine.device_metric_sums(X, Y), engine.device_wasserstein(X, Y)
    assert sums.shape == ref_s.shape and w1.shape == ref_w.shape
    assert torch.allclose(sums, ref_s, rtol=1e-12, atol=0), (sums - ref_s).abs().max()
    assert torch.allclose(w1, ref_w, rtol=1e-12, atol=1e-18), (w1 - ref_w).abs().max()
    # against numpy's own sort for one (pair, step)
    u, v = np.sort(X[n - 1, B - 1].cpu().numpy()).astype(np.float64), np.sort(Y[n - 1, B - 1].cpu().numpy()).astype(np.float64)
    assert abs(w1[B - 1, n - 1].item() - np.abs(u - v).mean()) <= 1e-12 * max(1.0, np.abs(u - v).mean())
    same_s, same_w = engine.device_pair_metrics(X, X)
    assert not same_w.cpu().numpy().any() and not same_s[..., 0].cpu().numpy().any()


def test_one_pass_pair_metrics_keep_non_finite_states_in_their_cell():
    """A NaN / Inf coordinate makes the terms of ITS (pair, step) and of the next step's differences non-finite, exactly where
    the separate kernels put them, and nowhere else."""
    n, B, E = 6, 4, 768
    g = torch.Generator().manual_seed(3)
    X = torch.randn(n, B, E, generator=g)
    Y = torch.randn(n, B, E, generator=g)
    X[2, 1, 100] = float("nan")
    Y[4, 3, 7] = float("inf")
    sums, w1 = engine.device_pair_metrics(X.to(DEV), Y.to(DEV))
    ref_s, ref_w = engine.device_metric_sums(X.to(DEV), Y.to(DEV)), engine.device_wasserstein(X.to(DEV), Y.to(DEV))
    assert torch.equal(torch.isfinite(sums), torch.isfinite(ref_s))
    # the exact class (NaN, +inf, -inf, finite) of every cell, both paths, against the float64 restatement
    want_s, _ = ref64.traj_metrics(X.numpy(), Y.numpy())
    want_w, _ = ref64.wasserstein(X.numpy(), Y.numpy())
    for got, want in ((sums, want_s), (ref_s, want_s), (w1, want_w), (ref_w, want_w)):
        assert np.array_equal(ref64.classes(got.cpu().numpy()), ref64.classes(want))
    bad = ~torch.isfinite(w1)
    assert torch.equal(bad, ~torch.isfinite(ref_w)) and bad[1, 2] and bad[3, 4] and bad.sum().item() == 2
    ok = torch.isfinite(ref_s)
    assert torch.allclose(sums[ok], ref_s[ok], rtol=1e-12, atol=0)
