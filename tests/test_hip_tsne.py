"""GPU: the device t-SNE (include/dt_hip_tsne.h, analysis/dimensionality/tsne.py) against the float64 yardstick
tests/tsne_ref64.py on the seeded problems of tests/tsne_cases.py.

The optimiser is chaotic (a 1e-15 relative change of the start reaches order 1 by iteration 100), so no long run is
compared element by element: steps are compared over 3 iterations from the yardstick's own states, long runs by their KL
divergence (within 3 s of tsne_cases.CHAOS_SPREAD above the yardstick's; a lower KL is a better optimum and passes)."""
import os

import numpy as np
import pytest
import torch

import tsne_cases as cases
import tsne_ref64 as ref
from distillation_trajectories_amd import engine
from distillation_trajectories_amd.analysis.dimensionality.tsne import (TrajectoryTSNE, pca_start, tsne_pairs,
                                                                         tsne_sweep)
from pca_ref64 import pca_ref64

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
STATE_KEYS = ("y", "update", "gains")


def _dev(x):
    return torch.tensor(np.asarray(x)).to(DEV)                     # a copy: the shared cases stay as they are


def _pack(states, n):
    """yardstick states -> the [P, 6 n + 4] fp64 state tensor of engine.device_tsne"""
    out = np.zeros((len(states), engine.tsne_state_doubles(n)))
    for p, s in enumerate(states):
        out[p, :6 * n] = np.concatenate([s[k].ravel() for k in STATE_KEYS])
        out[p, 6 * n:] = (s["best_error"], s["best_iter"], s["n_iter"], s["stop"])
    return _dev(out)


def _views(r, n, p=0):
    v = engine.tsne_state_views(r["state"], n)
    return {k: v[k][p].cpu().numpy() for k in STATE_KEYS + ("ctl",)}


def _schedule(c, **over):
    prm = dict(c["params"], **over)
    return dict(early_exaggeration=prm["early_exaggeration"], exaggeration_iters=prm["exaggeration_iters"],
                learning_rate=prm["learning_rate"], momentum=prm["momentum"], min_gain=prm["min_gain"],
                n_iter_check=prm["n_iter_check"], n_iter_without_progress=prm["n_iter_without_progress"],
                min_grad_norm=prm["min_grad_norm"])


# ------------------------------------------------------------------------------------------------ affinities
@pytest.mark.parametrize("shape", [(4, 4), (12, 12), (65, 48), (102, 768), (130, 48), (512, 16)], ids=lambda s: f"n{s[0]}")
def test_affinities_match_the_yardstick(shape):
    """perplexities 1.5, the reference's min(30, n // 5) and n - 1.5, to 1e-10 of max P.  At n = 4 the reference's rule
    gives perplexity 0, which is outside 0 < perplexity < n: that case must be refused."""
    n, E = shape
    X = ref.walk_pair(40 + n, n, E)
    Y0 = np.zeros((n, 2))
    D = ref.sq_distances(X)
    for perp in (1.5, float(min(30, n // 5)), n - 1.5):
        if perp == 0.0:
            with pytest.raises(ValueError, match="perplexity"):
                engine.device_tsne(_dev(X), perplexity=perp, init=Y0, max_iter=0)
            continue
        r = engine.device_tsne(_dev(X[: n // 2]), _dev(X[n // 2:]), perplexity=perp, init=Y0, max_iter=0,
                               return_affinities=True)
        got, want = r["affinities"][0].cpu().numpy(), ref.joint(ref.conditional(D, perp))
        gap = np.abs(got - want).max() / want.max()
        print(shape, perp, "affinity gap / max P", gap)
        assert r["status"].tolist() == [0] and r["n_iter"].tolist() == [0]
        assert gap <= 1e-10, (shape, perp)
        assert np.array_equal(got, got.T) and np.all(np.diag(got) == 0.0)


def test_affinities_of_a_golden_pair(golden):
    arrays, _ = golden
    t, s = arrays["pair0_teacher"], arrays["pair0_student"]
    X = np.vstack([t.reshape(len(t), -1), s.reshape(len(s), -1)])
    n = len(X)
    r = engine.device_tsne(_dev(t.reshape(len(t), -1)), _dev(s.reshape(len(s), -1)), perplexity=min(30, n // 5),
                           init=np.zeros((n, 2)), max_iter=0, return_affinities=True)
    want = ref.affinities(X, min(30, n // 5))
    assert np.abs(r["affinities"][0].cpu().numpy() - want).max() <= 1e-10 * want.max()


def test_nan_rows_give_status_1_and_nan_outputs_for_that_problem_only():
    n, E = 20, 16
    X = np.stack([ref.walk_pair(70 + p, n, E) for p in range(3)], axis=1)          # step-major [n, 3, E]
    Y0 = 1e-4 * np.random.RandomState(9).standard_normal((n, 2))
    clean = engine.device_tsne(_dev(X), perplexity=4.0, init=Y0, max_iter=30, return_affinities=True)
    Xb = X.copy()
    Xb[7, 1, 5] = np.nan
    bad = engine.device_tsne(_dev(Xb), perplexity=4.0, init=Y0, max_iter=30, return_affinities=True)
    assert clean["status"].tolist() == [0, 0, 0] and bad["status"].tolist() == [0, 1, 0]
    for key in ("embedding", "kl_divergence", "affinities"):
        assert torch.isnan(bad[key][1]).all(), key
        for p in (0, 2):
            assert torch.equal(bad[key][p], clean[key][p]), (key, p)
    assert bad["n_iter"].tolist() == [30, 0, 30]
    with pytest.raises(ValueError, match="NaN or infinity"):
        TrajectoryTSNE(perplexity=4.0, init="random", random_state=0, max_iter=10).fit(Xb[:, 1])


# ------------------------------------------------------------------------------------------------ steps
@pytest.mark.parametrize("shape", [(102, 768), (65, 48)], ids=lambda s: f"n{s[0]}")
def test_three_steps_from_the_yardsticks_states(shape):
    """From the yardstick's state before iterations 0, 5, 249, 250 and 600, 3 device iterations on the yardstick's own
    affinities: y, update and gains within 1e-10 of their max-abs, the plain KL within 1e-10 relative.  No gain decision
    of these iterations is near a tie (tie_margin, checked on the yardstick's side)."""
    n, E = shape
    c = cases.case(n, E)
    assert c["tie_margin"] >= 1e-9, c["tie_margin"]
    X, P = _dev(c["X"]), _dev(c["P"])[None]
    for it in (0, 5, 249, 250, 600):
        want = ref.descend(c["states"][it], c["P"], it, it + 3, c["params"])
        r = engine.device_tsne(X, perplexity=c["perplexity"], state=_pack([c["states"][it]], n), it_begin=it,
                               max_iter=it + 3, affinities=P, **_schedule(c))
        got = _views(r, n)
        for key in STATE_KEYS:
            gap = np.abs(got[key] - want[key]).max() / np.abs(want[key]).max()
            print(shape, it, key, gap)
            assert gap <= 1e-10, (shape, it, key, gap)
        kl_want = ref.final_kl(want, c["P"])
        assert abs(r["kl_divergence"].item() - kl_want) <= 1e-10 * kl_want, (shape, it)
        assert got["ctl"][2] == it + 3 and got["ctl"][3] == 0 and r["n_iter"].item() == it + 3
        assert got["ctl"][1] == want["best_iter"] and got["ctl"][0] == want["best_error"]      # no check, or a reset after it
        assert np.array_equal(r["embedding"][0].cpu().numpy(), got["y"].astype(np.float32))
    # best_error across a check: iterations 48 .. 50 hold the check of iteration 49
    s48 = ref.descend(c["states"][5], c["P"], 5, 48, c["params"])
    assert cases.tie_margin(s48, c["P"], 48, 51, c["params"]) >= 1e-9
    want = ref.descend(s48, c["P"], 48, 51, c["params"])
    r = engine.device_tsne(X, perplexity=c["perplexity"], state=_pack([s48], n), it_begin=48, max_iter=51, affinities=P,
                           **_schedule(c))
    ctl = _views(r, n)["ctl"]
    assert ctl[1] == want["best_iter"] == 49 and abs(ctl[0] - want["best_error"]) <= 1e-10 * want["best_error"]


def test_three_steps_with_a_whole_wave_per_row():
    """n = 130 takes the 64-lane row groups (n <= 128 takes 16): the same check from a mid-run state"""
    n, E = 130, 48
    c = cases.case(n, E)
    s = ref.descend(ref.new_state(c["Y0"]), c["P"], 0, 30, c["params"])
    assert cases.tie_margin(s, c["P"], 30, 33, c["params"]) >= 1e-9
    want = ref.descend(s, c["P"], 30, 33, c["params"])
    r = engine.device_tsne(_dev(c["X"]), perplexity=c["perplexity"], state=_pack([s], n), it_begin=30, max_iter=33,
                           affinities=_dev(c["P"])[None], **_schedule(c))
    got = _views(r, n)
    for key in STATE_KEYS:
        assert np.abs(got[key] - want[key]).max() <= 1e-10 * np.abs(want[key]).max(), key
    kl_want = ref.final_kl(want, c["P"])
    assert abs(r["kl_divergence"].item() - kl_want) <= 1e-10 * kl_want


# ------------------------------------------------------------------------------------------------ resume, batch
@pytest.mark.parametrize("exaggeration_iters", [250, 20])
def test_resume_gives_the_same_bits(exaggeration_iters):
    c = cases.case(65, 48)
    X = _dev(c["X"])
    kw = dict(perplexity=c["perplexity"], exaggeration_iters=exaggeration_iters, n_iter_check=10)
    whole = engine.device_tsne(X, init=c["Y0"], max_iter=40, **kw)
    first = engine.device_tsne(X, init=c["Y0"], max_iter=17, **kw)
    second = engine.device_tsne(X, state=first["state"], it_begin=17, max_iter=40, **kw)
    assert first["n_iter"].item() == 17 and second["n_iter"].item() == 40
    for key in ("state", "embedding", "kl_divergence", "n_iter"):
        assert torch.equal(whole[key], second[key]), key
    assert not torch.equal(first["state"], second["state"])               # the state given is left as it was


def test_a_problems_bits_do_not_depend_on_the_batch_or_the_strides():
    n, E, S = 65, 48, 7
    X = np.stack([ref.walk_pair(200 + p, n, E) for p in range(S)], axis=1)          # step-major [n, S, E]
    Xd = _dev(X)
    a, b = Xd[:33], Xd[33:]
    Y0 = cases.start(65, 48)
    kw = dict(perplexity=13.0, init=Y0, max_iter=60)
    batch = engine.device_tsne(a, b, **kw)
    for p in (0, 6):
        assert not a[:, p].is_contiguous()
        runs = {"in place": engine.device_tsne(a[:, p], b[:, p], **kw),
                "packed": engine.device_tsne(a[:, p].contiguous(), b[:, p].contiguous(), **kw),
                "one set": engine.device_tsne(Xd[:, p].contiguous(), **kw)}
        for name, r in runs.items():
            for key in ("embedding", "kl_divergence", "state"):
                assert torch.equal(r[key][0], batch[key][p]), (p, name, key)
    moved = engine.device_tsne(torch.flip(a, dims=[1]), torch.flip(b, dims=[1]), **kw)       # problem 0 as problem 6
    for key in ("embedding", "kl_divergence", "state"):
        assert torch.equal(moved[key][6], batch[key][0]) and torch.equal(moved[key][0], batch[key][6]), key


# ------------------------------------------------------------------------------------------------ stop rules
def test_stop_rules():
    n, E = 65, 48
    c = cases.case(n, E)
    X = np.stack([c["X"], ref.walk_pair(300, n, E), ref.walk_pair(301, n, E)], axis=1)
    quick = engine.device_tsne(_dev(X), perplexity=c["perplexity"], init=c["Y0"], max_iter=1000, min_grad_norm=1e300)
    assert quick["n_iter"].tolist() == [50, 50, 50]
    assert engine.tsne_state_views(quick["state"], n)["ctl"][:, 3].tolist() == [ref.GRAD_NORM] * 3

    stuck = dict(ref.copy_state(c["states"][300]), best_error=0.0, best_iter=-1)
    P = _dev(c["P"])[None]
    kw = dict(perplexity=c["perplexity"], affinities=P, **_schedule(c))
    r = engine.device_tsne(_dev(c["X"]), state=_pack([stuck], n), it_begin=300, max_iter=1000, **kw)
    ctl = _views(r, n)["ctl"]
    assert r["n_iter"].item() == 350 and ctl[3] == ref.NO_PROGRESS and ctl[0] == 0.0 and ctl[1] == -1.0
    more = engine.device_tsne(_dev(c["X"]), state=r["state"], it_begin=350, max_iter=1000, **kw)
    for key in ("state", "embedding", "kl_divergence", "n_iter"):
        assert torch.equal(more[key], r[key]), key


# ------------------------------------------------------------------------------------------------ full run
@pytest.mark.parametrize("shape", [(102, 768), (130, 48)], ids=lambda s: f"n{s[0]}")
def test_full_run_reaches_the_yardsticks_kl(shape):
    """1000 iterations, default schedule, from the stored Y0.  The reported KL is that of the returned y (1e-9 relative,
    recomputed in float64 on the host from the device's own affinities) and at most KL_ref (1 + 3 s): KL_ref the
    yardstick's from the same Y0, s = tsne_cases.CHAOS_SPREAD (8.1e-4 at n = 102, 7.3e-3 at n = 130).  No lower bound."""
    n, E = shape
    c = cases.case(n, E)
    r = engine.device_tsne(_dev(c["X"]), perplexity=c["perplexity"], init=c["Y0"], max_iter=1000, return_affinities=True)
    assert r["n_iter"].item() == 1000 and r["status"].item() == 0
    y = _views(r, n)["y"]
    kl = r["kl_divergence"].item()
    kl_host = ref.kl_grad(y, r["affinities"][0].cpu().numpy())[0]
    kl_ref = ref.final_kl(c["final"], c["P"])
    bound = kl_ref * (1.0 + cases.CHAOS_FACTOR * cases.CHAOS_SPREAD[shape])
    print(shape, "KL device", kl, "recomputed", kl_host, "yardstick", kl_ref, "bound", bound)
    assert abs(kl - kl_host) <= 1e-9 * kl_host
    assert kl <= bound
    assert np.array_equal(r["embedding"][0].cpu().numpy(), y.astype(np.float32))


# ------------------------------------------------------------------------------------------------ public layer
def test_trajectory_tsne_equals_the_engine_call_and_starts_from_the_pca():
    c = cases.case(65, 48)
    r = engine.device_tsne(_dev(c["X"]), perplexity=c["perplexity"], init=c["Y0"], max_iter=120)
    t = TrajectoryTSNE(perplexity=c["perplexity"], init=c["Y0"], max_iter=120)
    emb = t.fit_transform(c["X"])
    assert isinstance(emb, np.ndarray) and np.array_equal(emb, r["embedding"][0].cpu().numpy())
    assert np.array_equal(t.embedding_, emb) and t.kl_divergence_ == r["kl_divergence"].item()
    assert t.n_iter_ == 120 and t.learning_rate_ == 50.0
    on_dev = TrajectoryTSNE(perplexity=c["perplexity"], init=c["Y0"], max_iter=120).fit_transform(_dev(c["X"]))
    assert on_dev.device == DEV and np.array_equal(on_dev.cpu().numpy(), emb)

    p = TrajectoryTSNE(perplexity=c["perplexity"], init="pca", max_iter=0).fit(c["X"])
    start = np.asarray(p.init_embedding_, np.float64)
    assert abs(start[:, 0].std() - 1e-4) <= 1e-10
    scores = pca_ref64(c["X"], 2)["scores"]
    want = scores / scores[:, 0].std() * 1e-4
    assert np.abs(start - want).max() <= 2e-6 * np.abs(want).max()
    assert np.array_equal(p.embedding_, start.astype(np.float32)) and p.n_iter_ == 0

    a = TrajectoryTSNE(perplexity=5.0, init="random", random_state=42, max_iter=0).fit(c["X"])
    want = 1e-4 * np.random.RandomState(42).standard_normal((65, 2)).astype(np.float32)
    assert np.array_equal(a.embedding_, want.astype(np.float32))


def test_tsne_pairs_equals_single_calls():
    n, E, S = 40, 32, 3
    X = _dev(np.stack([ref.walk_pair(400 + p, n, E) for p in range(S)], axis=1))
    a, b = X[:20].reshape(20, S, 2, 4, 4), X[20:].reshape(20, S, 2, 4, 4)
    start = pca_start(a.reshape(20, S, -1), b.reshape(20, S, -1))
    many = tsne_pairs(a, b, 8, start, max_iter=80)
    assert many["embedding"].shape == (S, n, 2)
    for s in range(S):
        one = engine.device_tsne(torch.cat([X[:20, s], X[20:, s]]), perplexity=8, init=start[s], max_iter=80)
        for key in ("embedding", "kl_divergence", "n_iter", "status"):
            assert torch.equal(one[key][0], many[key][s]), (s, key)


def _tuple_traj(states):
    """the reference's trajectory format: a list of (x [1, C, H, W], t) tuples"""
    return [(torch.from_numpy(states[i]), 50 - i) for i in range(len(states))]


def test_mirror_driver_writes_tsne_next_to_pca(golden, tmp_path, capsys):
    from distillation_trajectories_amd.analysis.dimensionality import dimensionality_reduction_analysis
    from distillation_trajectories_amd.analysis.dimensionality.dimensionality_reduction import joint_pca
    from distillation_trajectories_amd.config import Config
    arrays, _ = golden
    cfg = Config(base_dir=str(tmp_path))
    teachers = [_tuple_traj(arrays[f"pair{i}_teacher"]) for i in range(4)]
    students = [_tuple_traj(arrays[f"pair{i}_student"]) for i in range(4)]
    students[1] = students[1][::2]
    out = dimensionality_reduction_analysis(teachers, students, cfg, size_factor=0.1)
    assert sorted(os.listdir(out)) == ["trajectory_0", "trajectory_1", "trajectory_2"]
    for i in range(3):
        d = os.path.join(out, f"trajectory_{i}")
        assert sorted(os.listdir(d)) == ["pca_trajectory.npz", "tsne_trajectory.npz"]
        got = np.load(os.path.join(d, "tsne_trajectory.npz"))
        assert got["teacher"].shape == (len(teachers[i]), 2) and got["student"].shape == (len(students[i]), 2)
        assert np.isfinite(got["teacher"]).all() and np.isfinite(got["student"]).all()
        assert got["kl_divergence"].shape == () and np.isfinite(got["kl_divergence"]) and got["kl_divergence"] > 0
        pca = np.load(os.path.join(d, "pca_trajectory.npz"))
        want = dict(zip(("teacher", "student", "explained_variance_ratio"), joint_pca(teachers[i], students[i], 2)))
        assert sorted(pca.files) == sorted(want)
        for key, w in want.items():
            assert pca[key].dtype == w.dtype and pca[key].tobytes() == w.tobytes(), (i, key)
    text = capsys.readouterr().out
    for i in range(3):
        assert f"  Performing PCA for trajectory {i}..." in text and f"  Performing t-SNE for trajectory {i}..." in text
    assert "Error performing" not in text and "too many points" not in text and "trajectory 3" not in text
    assert text.count("UMAP") == 3


def test_mirror_driver_skips_tsne_above_500_rows(tmp_path, capsys):
    from distillation_trajectories_amd.analysis.dimensionality import dimensionality_reduction_analysis
    from distillation_trajectories_amd.config import Config
    rows = ref.walk_pair(500, 501, 4).reshape(501, 1, 1, 2, 2)
    cfg = Config(base_dir=str(tmp_path))
    out = dimensionality_reduction_analysis([_tuple_traj(rows[:251])], [_tuple_traj(rows[251:])], cfg)
    assert os.listdir(os.path.join(out, "trajectory_0")) == ["pca_trajectory.npz"]
    text = capsys.readouterr().out
    assert "  Skipping t-SNE for trajectory 0 (too many points)" in text and "Performing t-SNE" not in text


def test_sweep_cell_matches_tsne_pairs():
    from distillation_trajectories_amd.analysis.trajectory_engine import sample_grid
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model, noise_table
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 10
    S, scales, T = 2, [1.0, 3.0], 10
    teacher = make_model(DiffusionUNet, cfg, 0.2).to(DEV)
    student = make_model(DiffusionUNet, cfg, 0.01).to(DEV)
    res = tsne_sweep(teacher, [student], cfg, scales, S, max_iter=100)
    n = 2 * (T + 1)
    assert res["embedding"].shape == (1, 2, S, n, 2) and res["kl_divergence"].shape == (1, 2, S)
    assert (res["status"] == 0).all() and (res["n_iter"] == 100).all() and np.isfinite(res["embedding"]).all()
    table = noise_table(42, S + T - 1, (1, 3, 16, 16)).reshape(S + T - 1, -1).to(DEV)
    t_grid = sample_grid(engine.UNetHandle.for_module(teacher), table, 0, S, T, scales, 16, 16)
    s_grid = sample_grid(engine.UNetHandle.for_module(student), table, 0, S, T, scales, 16, 16)
    for g, gs in enumerate(scales):
        want = tsne_pairs(t_grid[gs], s_grid[gs], min(30, n // 5), pca_start(t_grid[gs], s_grid[gs]), max_iter=100)
        assert np.array_equal(res["embedding"][0, g], want["embedding"].cpu().numpy()), gs
        assert np.array_equal(res["kl_divergence"][0, g], want["kl_divergence"].cpu().numpy()), gs
