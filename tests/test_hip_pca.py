"""GPU: the device PCA (include/dt_hip_pca.h, analysis/dimensionality/) against the float64 yardstick pca_ref64 (numpy SVD
of the centred float64 rows, sklearn's sign rule), on the golden trajectory pairs and on seeded random walks; batch
independence and repeatability bit for bit; the status words; the projection; the reference's mirror drivers; the sweep."""
import os

import numpy as np
import pytest
import torch

from distillation_trajectories_amd import engine
from distillation_trajectories_amd.analysis.dimensionality.pca import TrajectoryPCA, pca_pairs, pca_sweep
from pca_cases import compare_vectors as _compare
from pca_ref64 import ambiguous_sign, pca_ref64

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
FIELDS = ("mean", "components", "scores", "singular_values", "explained_variance", "explained_variance_ratio")


def _walk(seed, n, P, E, scale=1.0):
    """seeded random-walk trajectories, step-major [n, P, E] fp32, with a large common offset (as trajectory states have)"""
    g = torch.Generator().manual_seed(seed)
    steps = torch.randn(n, P, E, generator=g, dtype=torch.float64) * scale
    return (steps.cumsum(0) + 5.0).float()


def _problem(r, p):
    return {f: r[f][p].cpu().numpy() for f in FIELDS}


def _rows(X, Y, p):
    return np.vstack([X[:, p].reshape(X.shape[0], -1).cpu().numpy(), Y[:, p].reshape(Y.shape[0], -1).cpu().numpy()])


def test_pca_entry_host_code_clean_under_asan_and_ubsan():
    """tests/host_sanitize/pca_driver.cpp (every entry of include/dt_hip_pca.h) under host ASan / UBSan."""
    import subprocess
    from distillation_trajectories_amd.csrc.build import PCA_SAN_DRIVER, build_pca_sanitizer_driver
    if not os.path.exists(PCA_SAN_DRIVER):
        build_pca_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([PCA_SAN_DRIVER], capture_output=True, text=True, env=env, timeout=300)
    report = r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, report
    assert r.returncode == 0 and "pca driver ok" in r.stdout, report


def test_golden_pairs_match_ref64(golden):
    arrays, _ = golden
    X = torch.from_numpy(np.concatenate([arrays[f"pair{i}_teacher"] for i in range(4)], axis=1)).reshape(51, 4, -1)
    Y = torch.from_numpy(np.concatenate([arrays[f"pair{i}_student"] for i in range(4)], axis=1)).reshape(51, 4, -1)
    r = engine.device_pca(X.to(DEV), 3, Y.to(DEV))
    assert r["status"].cpu().tolist() == [0, 0, 0, 0]
    for p in range(4):
        _compare(_problem(r, p), pca_ref64(_rows(X, Y, p), 3), 3, f"pair{p}")


@pytest.mark.parametrize("shape", [
    dict(nx=101, ny=101, E=3072, P=3, k=2),      # the default config: T = 100, 32 x 32 x 3
    dict(nx=51, ny=26, E=768, P=3, k=3),         # unequal lengths
    dict(nx=51, ny=51, E=784, P=2, k=4),         # 1 x 28 x 28
    dict(nx=51, ny=0, E=768, P=2, k=3),          # a single set
    dict(nx=26, ny=26, E=675, P=2, k=16),        # 3 x 15 x 15: E padded to a multiple of 4
    dict(nx=2002, ny=0, E=768, P=1, k=3),        # T = 1000 at 16 x 16 x 3, one problem
    dict(nx=33, ny=32, E=36, P=2, k=3),          # n = 65: one row into the second tile; the last stage holds one quad
    dict(nx=65, ny=64, E=20, P=2, k=3),          # n = 129: three tile rows, mirrored off-diagonal tiles
    dict(nx=64, ny=0, E=64, P=1, k=2),           # exactly one tile
], ids=["default", "unequal", "mnist", "single", "pad", "n2002", "n65", "n129", "one_tile"])
def test_shapes_match_ref64(shape):
    nx, ny, E, P, k = shape["nx"], shape["ny"], shape["E"], shape["P"], shape["k"]
    X = _walk(11 + nx, nx, P, E)
    Y = _walk(12 + ny, ny, P, E, 0.8) if ny else None
    r = engine.device_pca(X.to(DEV), k, None if Y is None else Y.to(DEV))
    assert (r["status"] == 0).all()
    for p in range(P):
        rows = _rows(X, Y, p) if ny else X[:, p].numpy()
        _compare(_problem(r, p), pca_ref64(rows, k), k, (shape, p))


def test_batch_independent_repeatable_and_stride_blind():
    X, Y = _walk(1, 41, 64, 768).to(DEV), _walk(2, 41, 64, 768).to(DEV)
    big = engine.device_pca(X, 3, Y)
    again = engine.device_pca(X, 3, Y)
    for f in FIELDS + ("status",):
        assert torch.equal(big[f], again[f]), f
    for p in (0, 17, 63):
        alone = engine.device_pca(X[:, p].contiguous(), 3, Y[:, p].contiguous())
        for f in FIELDS:
            assert torch.equal(alone[f][0], big[f][p]), (p, f)
    # a strided step-major view (every other problem) against a contiguous copy of it
    Xs, Ys = X[:, ::2], Y[:, ::2]
    assert not Xs.is_contiguous()
    strided, copied = engine.device_pca(Xs, 3, Ys), engine.device_pca(Xs.contiguous(), 3, Ys.contiguous())
    for f in FIELDS:
        assert torch.equal(strided[f], copied[f]), f
        assert torch.equal(strided[f], big[f][::2]), f


def test_status_words_isolate_bad_problems():
    X, Y = _walk(3, 21, 8, 256), _walk(4, 21, 8, 256)
    clean = engine.device_pca(X.to(DEV), 2, Y.to(DEV))
    Xb = X.clone()
    Xb[7, 2, 100] = float("nan")
    Xb[:, 5] = 0.25                                            # problem 5: constant rows
    Yb = Y.clone()
    Yb[:, 5] = 0.25
    bad = engine.device_pca(Xb.to(DEV), 2, Yb.to(DEV))
    assert bad["status"].cpu().tolist() == [0, 0, 1, 0, 0, 2, 0, 0]
    for p in (0, 1, 3, 4, 6, 7):
        for f in FIELDS:
            assert torch.equal(bad[f][p], clean[f][p]), (p, f)
    for f in FIELDS:
        assert torch.isnan(bad[f][2]).all(), f
    z = _problem(bad, 5)
    assert np.all(z["singular_values"] == 0) and np.all(z["explained_variance"] == 0)
    assert np.all(np.isnan(z["explained_variance_ratio"]))
    assert np.all(z["scores"] == 0) and np.all(z["components"] == 0)
    assert np.allclose(z["mean"], 0.25)
    with pytest.raises(ValueError, match="NaN or infinity"):
        TrajectoryPCA(2).fit(torch.cat([Xb[:, 2], Yb[:, 2]]).to(DEV))
    with pytest.warns(RuntimeWarning, match="zero total variance"):
        pca = TrajectoryPCA(2).fit(torch.cat([Xb[:, 5], Yb[:, 5]]).numpy())
    assert np.all(np.isnan(pca.explained_variance_ratio_))


def test_project_reproduces_fit_and_the_fit_on_one_flow():
    X, Y = _walk(5, 31, 6, 512).to(DEV), _walk(6, 25, 6, 512).to(DEV)
    r = engine.device_pca(X, 3, Y)
    proj = engine.device_pca_project(X, r["mean"], r["components"], Y)
    scale = r["scores"].abs().amax(dim=(1, 2), keepdim=True)
    assert ((proj - r["scores"]).abs() / scale).max().item() <= 1e-6
    # scripts/analysis/analyze_trajectories.py: fit on the first scale's averaged trajectory, transform every scale's
    trajs = [_walk(20 + g, 51, 1, 768)[:, 0] for g in range(3)]
    pca = TrajectoryPCA(3).fit(trajs[0].numpy())
    ref = pca_ref64(trajs[0].numpy(), 3)
    _compare({"mean": pca.mean_, "components": pca.components_, "scores": pca.transform(trajs[0].numpy()),
              "singular_values": pca.singular_values_, "explained_variance": pca.explained_variance_,
              "explained_variance_ratio": pca.explained_variance_ratio_}, ref, 3, "fit")
    stacked = torch.stack(trajs, dim=1).to(DEV)                 # [51, 3 scales, E]: one shared basis for every scale
    all_scores = engine.device_pca_project(stacked, pca._mean_dev, pca._comp_dev)
    for g, t in enumerate(trajs):
        want = (t.numpy().astype(np.float64) - ref["mean"]) @ ref["components"].T
        got = all_scores[g].cpu().numpy()
        assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max(), g
        assert np.array_equal(got, pca.transform(t.to(DEV)).cpu().numpy())


def _tuple_traj(states):
    """the reference's trajectory format: a list of (x [1, C, H, W], t) tuples"""
    return [(torch.from_numpy(states[i]), 50 - i) for i in range(len(states))]


def test_mirror_drivers_on_golden_pairs(golden, tmp_path, capsys):
    from distillation_trajectories_amd.analysis.dimensionality import (dimensionality_reduction_analysis,
                                                                       generate_latent_space_visualization)
    from distillation_trajectories_amd.config import Config
    arrays, _ = golden
    cfg = Config(base_dir=str(tmp_path))
    teachers = [_tuple_traj(arrays[f"pair{i}_teacher"]) for i in range(4)]
    students = [_tuple_traj(arrays[f"pair{i}_student"]) for i in range(4)]
    students[1] = students[1][::2]                              # unequal lengths are allowed
    out = dimensionality_reduction_analysis(teachers, students, cfg, size_factor=0.1)
    assert out == os.path.abspath(os.path.join(cfg.dimensionality_dir, "size_0.1"))
    assert sorted(os.listdir(out)) == ["trajectory_0", "trajectory_1", "trajectory_2"]
    for i in range(3):
        got = np.load(os.path.join(out, f"trajectory_{i}", "pca_trajectory.npz"))
        t_rows = np.stack([x[0].reshape(-1).numpy() for x in teachers[i]])
        s_rows = np.stack([x[0].reshape(-1).numpy() for x in students[i]])
        ref = pca_ref64(np.vstack([t_rows, s_rows]), 2)
        for j in range(2):
            sign = 1.0 if np.sign(got["teacher"][0, j]) == np.sign(ref["scores"][0, j]) or not ambiguous_sign(ref["components"][j]) else -1.0
            full = sign * np.concatenate([got["teacher"][:, j], got["student"][:, j]])
            assert np.abs(full - ref["scores"][:, j]).max() <= 2e-6 * np.abs(ref["scores"][:, j]).max(), (i, j)
        assert got["teacher"].shape == (len(t_rows), 2) and got["student"].shape == (len(s_rows), 2)
        assert np.abs(got["explained_variance_ratio"] - ref["explained_variance_ratio"]).max() <= 1e-9
    text = capsys.readouterr().out
    assert "Performing dimensionality reduction analysis for size factor 0.1..." in text
    assert "  Performing PCA for trajectory 2..." in text and "trajectory 3" not in text
    assert "Dimensionality reduction analysis completed for size factor 0.1" in text

    one = generate_latent_space_visualization(teachers[0], students[0], cfg, size_factor=0.1)
    first = dict(np.load(os.path.join(one, "latent_space.npz")))
    many = generate_latent_space_visualization(teachers, students, cfg, size_factor=0.1)
    second = dict(np.load(os.path.join(many, "latent_space.npz")))
    assert one == many == os.path.abspath(os.path.join(cfg.latent_space_dir, "size_0.1"))
    for key in ("teacher", "student", "explained_variance_ratio"):
        assert np.array_equal(first[key], second[key]), key
    ref = pca_ref64(np.vstack([np.stack([x[0].reshape(-1).numpy() for x in tr]) for tr in (teachers[0], students[0])]), 3)
    assert np.abs(first["explained_variance_ratio"] - ref["explained_variance_ratio"]).max() <= 1e-9


def test_sweep_matches_per_sample_fits():
    from distillation_trajectories_amd.analysis.trajectory_engine import sample_grid
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model, noise_table
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 50
    S, scales = 8, [1.0, 3.0]
    teacher = make_model(DiffusionUNet, cfg, 1.0).to(DEV)
    students = [make_model(DiffusionUNet, cfg, sf).to(DEV) for sf in (0.1, 0.5)]
    res = pca_sweep(teacher, students, cfg, scales, S, n_components=2)
    assert res["scores"].shape == (2, 2, S, 102, 2) and res["components"].shape == (2, 2, S, 2, 768)
    assert (res["status"] == 0).all()
    table = noise_table(42, S + 49, (1, 3, 16, 16)).reshape(S + 49, -1).to(DEV)
    t_grid = sample_grid(engine.UNetHandle.for_module(teacher), table, 0, S, 50, scales, 16, 16)
    for i, m in enumerate(students):
        s_grid = sample_grid(engine.UNetHandle.for_module(m), table, 0, S, 50, scales, 16, 16)
        for g, gs in enumerate(scales):
            for s in range(S):
                rows = torch.cat([t_grid[gs][:, s], s_grid[gs][:, s]])
                pca = TrajectoryPCA(2)
                scores = pca.fit_transform(rows)
                assert np.array_equal(scores.cpu().numpy(), res["scores"][i, g, s]), (i, gs, s)
                assert np.array_equal(pca.components_, res["components"][i, g, s])
                assert np.array_equal(pca.singular_values_, res["singular_values"][i, g, s])
                if s < 2 and g == 1:
                    got = {f: res[f][i, g, s] for f in FIELDS}
                    _compare(got, pca_ref64(rows.cpu().numpy(), 2), 2, (i, gs, s))
