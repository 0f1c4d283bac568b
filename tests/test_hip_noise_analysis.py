"""GPU: the noise-prediction driver and the teacher-shared sweep (analysis/noise_prediction/noise_analysis.py) against the
reference's own ``analyze_noise_prediction`` run (tests/golden/make_golden_noise.py) and against torch arithmetic."""
import json
import os

import numpy as np
import pytest
import torch

from distillation_trajectories_amd.analysis.noise_prediction import noise_analysis as na
from distillation_trajectories_amd.synthetic import state_dict_digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_noise():
    arrays = np.load(os.path.join(GOLDEN, "reference_vectors_noise.npz"))
    with open(os.path.join(GOLDEN, "reference_vectors_noise.json")) as f:
        meta = json.load(f)
    return arrays, meta


def _config(T):
    from distillation_trajectories_amd.config import Config
    c = Config()
    c.image_size, c.timesteps = 16, T
    return c


@pytest.fixture(scope="module")
def gpu_model():
    """Seeded synthetic models on the GPU, keyed by (size factor, fused path allowed)."""
    from distillation_trajectories_amd import engine
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model
    cache = {}

    def get(sf, fused=True):
        if (sf, fused) not in cache:
            m = make_model(DiffusionUNet, _config(50), sf).to(DEV)
            if not fused:
                engine.UNetHandle.for_module(m).set_fused(False)
            cache[(sf, fused)] = m
        return cache[(sf, fused)]
    return get


def test_noise_entry_host_code_clean_under_asan_and_ubsan():
    """tests/host_sanitize/noise_driver.cpp (every entry of include/dt_hip_noise.h) under host ASan / UBSan."""
    import subprocess
    from distillation_trajectories_amd.csrc.build import NOISE_SAN_DRIVER, build_noise_sanitizer_driver
    if not os.path.exists(NOISE_SAN_DRIVER):
        build_noise_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([NOISE_SAN_DRIVER], capture_output=True, text=True, env=env, timeout=300)
    report = r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, report
    assert r.returncode == 0 and "noise driver ok" in r.stdout, report


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


def test_q_sample_bit_identical_to_torch():
    from distillation_trajectories_amd import engine
    g = torch.Generator().manual_seed(5)
    for G, B, shape in ((1, 1, (3, 16, 16)), (7, 5, (3, 16, 16)), (13, 3, (3, 32, 32))):
        x0 = torch.randn(B, *shape, generator=g) * 3
        z = torch.randn(G, B, *shape, generator=g)
        ab = torch.rand(G, generator=g).clamp_min(1e-6)
        coef = torch.stack([torch.sqrt(ab), torch.sqrt(1 - ab)], dim=1)
        want = torch.stack([coef[i, 0] * x0 + coef[i, 1] * z[i] for i in range(G)])
        got = engine.q_sample(x0.to(DEV), z.to(DEV), coef.to(DEV)).cpu()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (G, B, shape)


@pytest.mark.parametrize("student_sf,conv_path", [(0.2, "fused"), (0.2, "layered"), (1.0, "layered")])
def test_internal_entry_matches_reference(golden_noise, gpu_model, student_sf, conv_path):
    from distillation_trajectories_amd import engine
    arrays, meta = golden_noise
    teacher = gpu_model(0.5)
    student = gpu_model(student_sf, fused=conv_path == "fused")
    assert engine.UNetHandle.for_module(student).fused_active(16, 16) == (conv_path == "fused")
    assert state_dict_digest(student.state_dict()) == meta["state_dict_sha256"][str(student_sf)]
    assert state_dict_digest(teacher.state_dict()) == meta["state_dict_sha256"]["0.5"]
    case = meta["cases"][str(student_sf)]
    t_list = meta["timesteps"]
    images = torch.from_numpy(arrays["images"]).to(DEV)
    noise = torch.from_numpy(arrays["noise"]).to(DEV)
    per_t, noised, _ = na._noise_prediction_metrics(teacher, student, images, t_list, noise, _config(meta["T"]))
    assert torch.equal(noised.cpu().view(torch.int32), torch.from_numpy(arrays["noised"]).view(torch.int32))
    by_t = {}
    for t, m in zip(t_list, per_t):
        by_t[t] = m
    for t, want in case["metrics_by_timestep"].items():
        for k, v in want.items():
            assert _rel(by_t[int(t)][k], v) < 1e-4, (t, k, by_t[int(t)][k], v)
    for key, k in (("avg_mse", "mse"), ("avg_mae", "mae"), ("avg_cosine_similarity", "cosine_similarity")):
        assert _rel(float(np.mean([m[k] for m in by_t.values()])), case[key]) < 1e-4, key


def test_driver_draws_noise_in_reference_order(golden_noise, gpu_model, tmp_path, capsys):
    arrays, meta = golden_noise
    teacher, student = gpu_model(0.5), gpu_model(0.2)
    images = torch.from_numpy(arrays["images"])
    cfg = _config(meta["T"])
    torch.manual_seed(77)
    res = na.analyze_noise_prediction(teacher, student, cfg, output_dir=str(tmp_path), size_factor=0.2, fixed_samples=images)
    after = torch.randn(4, device=DEV)
    console = capsys.readouterr().out
    torch.manual_seed(77)
    dev_images = images.to(DEV)
    noise = [torch.randn_like(dev_images) for _ in range(10)]
    assert torch.equal(torch.randn(4, device=DEV), after)            # the generator ends where the reference's would
    per_t, _, _ = na._noise_prediction_metrics(teacher, student, dev_images, meta["timesteps"], noise, cfg)
    assert list(res["metrics_by_timestep"]) == meta["timesteps"]
    for t, m in zip(meta["timesteps"], per_t):
        assert res["metrics_by_timestep"][t] == m
    assert res["avg_mse"] == np.mean([m["mse"] for m in per_t])
    with open(tmp_path / "noise_metrics_size_0.2.txt") as f:
        assert f.read() == na.format_noise_metrics(res)
    lines = console.splitlines()
    ref_lines = meta["cases"]["0.2"]["console"].splitlines()
    assert lines[:2] == ["Analyzing noise prediction for size factor 0.2...", "Using 6 fixed samples for consistent comparison"]
    assert lines[:2] == ref_lines[:2]
    assert lines[-1] == f"  Average Cosine Similarity: {res['avg_cosine_similarity']:.6f}"
    assert [ln.split(":")[0] for ln in lines[-3:]] == [ln.split(":")[0] for ln in ref_lines[-3:]]


def test_sweep_matches_driver_at_driver_timesteps(gpu_model, tmp_path):
    teacher = gpu_model(0.5)
    students = {0.2: gpu_model(0.2), 1.0: gpu_model(1.0)}
    cfg = _config(20)
    images = torch.rand(6, 3, 16, 16, generator=torch.Generator().manual_seed(3)) * 2 - 1
    t_list = torch.linspace(0, 19, 10, dtype=torch.long).tolist()
    torch.manual_seed(11)
    sweep = na.noise_prediction_sweep(teacher, students, images, timesteps=t_list, config=cfg)
    for sf, m in students.items():
        torch.manual_seed(11)
        res = na.analyze_noise_prediction(teacher, m, cfg, output_dir=str(tmp_path), size_factor=sf, fixed_samples=images)
        for t in t_list:
            for k in ("mse", "mae", "cosine_similarity"):
                assert _rel(sweep[sf][t][k], res["metrics_by_timestep"][t][k]) < 1e-4, (sf, t, k)


def test_sweep_student_independent_of_company_and_dense(gpu_model):
    teacher = gpu_model(0.5)
    everyone = {0.01: gpu_model(0.01), 0.2: gpu_model(0.2), 1.0: gpu_model(1.0)}
    cfg = _config(60)
    images = torch.rand(10, 3, 16, 16, generator=torch.Generator().manual_seed(4)) * 2 - 1
    full = na.noise_prediction_sweep(teacher, everyone, images, seed=9, config=cfg)      # 60 t x 10 images: two chunks
    for sf in everyone:
        assert sorted(full[sf]) == list(range(60))
    alone = na.noise_prediction_sweep(teacher, {0.2: everyone[0.2]}, images, seed=9, config=cfg)
    assert alone[0.2] == full[0.2]
    for t in (0, 30, 59):
        assert set(full[0.2][t]) == {"mse", "mae", "cosine_similarity", "teacher_true_mse", "student_true_mse"}
        assert full[0.2][t]["teacher_true_mse"] == full[1.0][t]["teacher_true_mse"]
    plain = na.noise_prediction_sweep(teacher, {0.2: everyone[0.2]}, images, timesteps=[5], seed=9, true_noise_metrics=False,
                                      config=cfg)
    assert set(plain[0.2][5]) == {"mse", "mae", "cosine_similarity"}


def test_sweep_true_noise_mse_against_torch(gpu_model):
    teacher, student = gpu_model(0.5), gpu_model(0.2)
    cfg = _config(30)
    images = (torch.rand(4, 3, 16, 16, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(DEV)
    t_list = [0, 13, 29]
    sweep = na.noise_prediction_sweep(teacher, {0.2: student}, images, timesteps=t_list, seed=21, config=cfg)
    gen = torch.Generator(device=DEV).manual_seed(21)
    noise = [torch.randn(images.shape, generator=gen, device=DEV) for _ in t_list]
    coef = na.noise_coefficients(cfg, t_list)
    for i, t in enumerate(t_list):
        x = coef[i, 0].to(DEV) * images + coef[i, 1].to(DEV) * noise[i]
        tt = torch.full((images.shape[0],), t, dtype=torch.long, device=DEV)
        et, es = teacher(x, tt).double(), student(x, tt).double()
        z = noise[i].double()
        assert _rel(sweep[0.2][t]["teacher_true_mse"], float(((et - z) ** 2).mean())) < 1e-4
        assert _rel(sweep[0.2][t]["student_true_mse"], float(((es - z) ** 2).mean())) < 1e-4
        assert _rel(sweep[0.2][t]["mse"], float(((et - es) ** 2).mean())) < 1e-4
