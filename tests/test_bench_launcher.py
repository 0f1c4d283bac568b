"""bench.py --gpus N must start its own N ranks (no torchrun) and relay rank 0's JSON line.

CPU-only: DT_BENCH_DRYRUN=1 stops each rank after the rendezvous + rank all-gather (gloo), so this
exercises the launcher, the environment it builds and the relay, not the GPU work.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = dict(os.environ, DT_BENCH_DRYRUN="1", **env)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True, text=True,
                          timeout=300)


def test_gpus_flag_spawns_that_many_ranks():
    res = _run(["--gpus", "3"])
    assert res.returncode == 0, res.stderr
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 3
    assert [r["rank"] for r in out["ranks"]] == [0, 1, 2]
    assert [r["local_rank"] for r in out["ranks"]] == [0, 1, 2]
    assert len({r["pid"] for r in out["ranks"]}) == 3 and os.getpid() not in {r["pid"] for r in out["ranks"]}


def test_single_rank_needs_no_launcher():
    out = json.loads(_run(["--gpus", "1"]).stdout.strip().splitlines()[-1])
    assert out["n_gpus"] == 1 and len(out["ranks"]) == 1


def test_failing_rank_fails_the_run():
    # without the dry-run switch the ranks refuse to run on a GPU-less host: the parent must report that
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "DT_BENCH_DRYRUN"):
        e.pop(k, None)
    e["CUDA_VISIBLE_DEVICES"] = e["HIP_VISIBLE_DEVICES"] = ""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=e, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode != 0
    assert "needs an MI355X" in res.stderr


def test_steps_must_be_positive():
    res = _run(["--steps", "0"])
    assert res.returncode != 0 and "--steps" in res.stderr


def test_dump_outputs_fit_the_limit_and_keep_the_same_rows(tmp_path):
    """--dump-outputs: float32 / float64 files within the byte limit, small outputs whole, a large one as the same seeded
    sample of its rows in every run, with the row numbers beside it."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    arrays = {"metric_mse": np.arange(256, dtype=np.float64), "counts": np.arange(5),
              "teacher_trajectory": torch.randn(51, 256, 768, generator=g), "student_trajectory": torch.randn(51, 256, 768, generator=g)}
    limit = 20 * 10**6
    shapes = bench.dump_outputs(arrays, str(tmp_path / "a"), limit)
    assert shapes == bench.dump_outputs(arrays, str(tmp_path / "b"), limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in shapes)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    assert np.array_equal(np.load(tmp_path / "a" / "metric_mse.npy"), arrays["metric_mse"])
    assert np.array_equal(np.load(tmp_path / "a" / "counts.npy"), np.arange(5.0))
    rows = np.load(tmp_path / "a" / "teacher_trajectory_rows.npy").astype(np.int64)
    assert 0 < len(rows) < 51 * 256 and np.all(np.diff(rows) > 0)
    want = arrays["teacher_trajectory"].reshape(-1, 768)[torch.from_numpy(rows)].numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "teacher_trajectory.npy"), want)


def test_dumped_metrics_are_finite_where_trajectory_mse_is_not():
    """Diverging pairs (1000 x mean step-MSE > 2, as for the benchmark's random-init models): trajectory_mse is NaN, so the
    dump writes its pre-transform trajectory_mse_pre instead, which determines it exactly."""
    import numpy as np
    import bench
    from distillation_trajectories_amd import engine
    rng = np.random.default_rng(0)
    n, E = 51, 768
    X = rng.standard_normal((n, 4, E)).cumsum(0)
    Y = X + rng.standard_normal((n, 4, E)) * np.array([0.001, 0.01, 1.0, 30.0])[None, :, None]
    sums = np.stack([((X - Y) ** 2).sum(-1), np.r_[np.zeros((1, 4)), (np.diff(X, axis=0) ** 2).sum(-1)],
                     np.r_[np.zeros((1, 4)), (np.diff(Y, axis=0) ** 2).sum(-1)],
                     np.r_[np.zeros((1, 4)), (np.diff(X, axis=0) * np.diff(Y, axis=0)).sum(-1)]], axis=-1).transpose(1, 0, 2)
    sums[:, 0, 3] = ((X[-1] - Y[-1]) ** 2).sum(-1)
    vals = engine.batch_scalar_metrics(sums, np.abs(sums[..., 0]), 256, E)
    assert np.isnan(vals["trajectory_mse"]).any() and np.isfinite(vals["trajectory_mse"]).any()
    keys = bench.dump_metrics()
    assert len(keys) == len(engine.SCALAR_KEYS) and "trajectory_mse" not in keys
    for k in keys:
        assert np.all(np.isfinite(vals[k])), k
    assert np.array_equal(vals["trajectory_mse"], np.log1p(1.0 - vals["trajectory_mse_pre"]), equal_nan=True)
