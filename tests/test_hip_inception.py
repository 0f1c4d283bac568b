"""GPU: the InceptionV3 feature extractor (include/dt_hip_inception.h, csrc/dt_inception.hip) against a float64
restatement of the network (tests/inception_ref.py), on random weights whose BatchNorm statistics are calibrated on that
restatement so that no layer is dead after its ReLU; batching and workspace invariance; the FID drivers."""
import os
import subprocess

import numpy as np
import pytest
import torch

import inception_ref as ref
from distillation_trajectories_amd import inception
from distillation_trajectories_amd.analysis.metrics import fid_score

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu

# bounds: per-image relative L2 error against float64, set just above the measured maxima
MODULE_TOL = 2e-6          # one module fed the device's own upstream output: measured max 1.40e-6 (Mixed_7b)
NETWORK_TOL = 2e-5         # preprocessing and all 19 modules: measured max 1.24e-5 (32x32, B=37, map (0.5, 0.5))

# channel slices of each concat (branch outputs in torchvision's order)
SLICES = {"Mixed_5b": [64, 64, 96, 32], "Mixed_5c": [64, 64, 96, 64], "Mixed_5d": [64, 64, 96, 64],
          "Mixed_6a": [384, 96, 288], "Mixed_7a": [320, 192, 768], "Mixed_7b": [320, 384, 384, 384, 384, 192],
          "Mixed_7c": [320, 384, 384, 384, 384, 192]}
for _m in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
    SLICES[_m] = [192, 192, 192, 192]


def _images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tanh(1.5 * torch.randn(n, 3, h, w, generator=g))


@pytest.fixture(scope="module")
def weights():
    """(float64 state dict, float32 state dict) with AuxLogits / fc / num_batches_tracked present."""
    sd = ref.random_state_dict(inception.key_table(), seed=11)
    ref.calibrate(sd, _images(4, 32, 32, seed=12).double(), 0.5, 0.5)
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    return sd, sd32


@pytest.fixture(scope="module")
def model(weights):
    return fid_score.InceptionModel(DEV, weights=weights[1])


def _rel_per_image(got, want):
    got, want = got.double().cpu().flatten(1), want.double().cpu().flatten(1)
    return ((got - want).norm(dim=1) / want.norm(dim=1)).numpy()


def test_inception_entry_host_code_clean_under_asan_and_ubsan():
    """tests/host_sanitize/inception_driver.cpp (every entry of include/dt_hip_inception.h) under host ASan / UBSan."""
    from distillation_trajectories_amd.csrc.build import INCEPTION_SAN_DRIVER, build_inception_sanitizer_driver
    if not os.path.exists(INCEPTION_SAN_DRIVER):
        build_inception_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([INCEPTION_SAN_DRIVER], capture_output=True, text=True, env=env, timeout=300)
    report = r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, report
    assert r.returncode == 0 and "inception driver ok" in r.stdout, report


def test_preprocess_matches_float64_resize_and_normalise(model):
    for h, w in ((16, 16), (24, 40), (299, 299), (1, 7)):
        imgs = _images(3, h, w, seed=h * 1000 + w)
        got = model.handle.preprocess(imgs, 0.5, 0.5).permute(0, 3, 1, 2)
        want = ref.preprocess(imgs.double(), 0.5, 0.5)
        err = (got.double().cpu() - want).abs().max().item()
        assert err <= 1e-5, f"preprocess {h}x{w}: max abs error {err:.3g}"


def test_every_module_on_its_own_upstream_output(weights, model):
    """Each module through the module-range entry, fed the device's own output of the module before; whole outputs
    (padding and concat slices included) and every concat slice against float64."""
    sd = weights[0]
    x = model.handle.preprocess(_images(5, 32, 32, seed=21), 0.5, 0.5)
    worst = {}
    for m, name in enumerate(inception.MODULES):
        y = model.handle.run_modules(x, m, m + 1)
        want = ref.run_module(sd, m, x.double().cpu().permute(0, 3, 1, 2))
        got = y if y.dim() == 2 else y.permute(0, 3, 1, 2)
        assert tuple(got.shape) == tuple(want.shape), name
        rel = _rel_per_image(got, want)
        worst[name] = float(rel.max())
        assert rel.max() <= MODULE_TOL, f"{name}: per-image relative L2 {rel.max():.3g}"
        c0 = 0
        for i, width in enumerate(SLICES.get(name, [])):
            r = _rel_per_image(got[:, c0:c0 + width], want[:, c0:c0 + width])
            assert r.max() <= MODULE_TOL, f"{name} concat slice {i} (channels {c0}..{c0 + width}): {r.max():.3g}"
            c0 += width
        x = y
    print("module maxima", {k: f"{v:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("hw", [(16, 16), (32, 32), (24, 40)])
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("in_map", [(0.5, 0.5), (1.0, 0.0)])
def test_whole_network_against_float64(weights, model, hw, B, in_map):
    imgs = _images(B, *hw, seed=B * 7 + hw[1])
    got = fid_score.extract_features(imgs, model, in_scale=in_map[0], in_shift=in_map[1])
    want = ref.features(weights[0], imgs.double(), *in_map)
    rel = _rel_per_image(got, want)
    print(f"network {hw} B={B} map={in_map}: max per-image relative L2 {rel.max():.2e}")
    assert rel.max() <= NETWORK_TOL, f"network {hw} B={B} {in_map}: {rel.max():.3g}"
    f = got.cpu()
    assert (f != 0).double().mean() > 0.75
    if B > 1:
        assert (f.std(dim=0) > 0).double().mean() > 0.9


def test_features_independent_of_batching_and_repeatable(model):
    imgs = _images(37, 24, 40, seed=5)
    full = fid_score.extract_features(imgs, model, batch_size=37)
    assert torch.equal(full, fid_score.extract_features(imgs, model, batch_size=37))
    for bs in (1, 5, 16):
        assert torch.equal(full, fid_score.extract_features(imgs, model, batch_size=bs)), bs
    other = torch.cat([_images(3, 24, 40, seed=6), imgs[10:11], _images(2, 24, 40, seed=7)])
    assert torch.equal(fid_score.extract_features(other, model)[3], full[10])


def test_poisoned_workspace_changes_nothing(model):
    imgs = _images(6, 32, 32, seed=8)
    want = fid_score.extract_features(imgs, model)
    ws = model.handle.workspace(6)
    for poison in (float("nan"), 1e30):
        ws.view(torch.float32).fill_(poison)
        assert torch.equal(fid_score.extract_features(imgs, model), want), poison
        x = model.handle.preprocess(imgs)
        ws.view(torch.float32).fill_(poison)
        assert torch.equal(model.handle.run_modules(x, 0, len(inception.MODULES)), want), poison


def test_get_features_chunks_of_32_equal_one_call(model):
    imgs = _images(40, 16, 16, seed=9)
    got = model.get_features(imgs)
    assert isinstance(got, np.ndarray) and got.shape == (40, 2048) and got.dtype == np.float32
    one = fid_score.extract_features(imgs, model, batch_size=40, in_scale=0.5, in_shift=0.5).cpu().numpy()
    assert np.array_equal(got, one)


def _diffusion_pair():
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model
    cfg = Config()
    cfg.image_size, cfg.timesteps, cfg.num_samples = 16, 6, 5
    return cfg, make_model(DiffusionUNet, cfg, 0.2).to(DEV), make_model(DiffusionUNet, cfg, 0.05).to(DEV)


def test_calculate_and_visualize_fid_driver(weights, tmp_path, capsys):
    cfg, teacher, student = _diffusion_pair()
    torch.manual_seed(31)
    res = fid_score.calculate_and_visualize_fid(teacher, student, cfg, output_dir=str(tmp_path), size_factor=0.05,
                                                weights=weights[1])
    out = capsys.readouterr().out
    torch.manual_seed(31)
    ts = fid_score.generate_samples(teacher, cfg, 5, DEV)
    ss = fid_score.generate_samples(student, cfg, 5, DEV)
    m = fid_score.InceptionModel(DEV, weights=weights[1])
    want = fid_score.calculate_fid(m.get_features(ts), m.get_features(ss))
    assert set(res) == {"fid_score"} and res["fid_score"] == want
    with open(tmp_path / "fid_score_size_0.05.txt", "rb") as f:
        assert f.read() == f"FID Score: {want:.4f}\n".encode()
    for line in ("Calculating FID scores for size factor 0.05...", "  Generating samples from teacher model...",
                 "  Generating samples from student model...", "  Extracting features using InceptionV3...",
                 "  Calculating FID score...", f"  FID score for size factor 0.05: {want:.4f}"):
        assert line in out.splitlines(), line


def test_compute_fid_agrees_with_calculate_fid(weights, model):
    from distillation_trajectories_amd.evaluation.metrics import compute_fid
    real = [(_images(1, 16, 16, seed=40 + i) + 1) / 2 for i in range(6)]
    gen = [(_images(1, 16, 16, seed=60 + i) + 1) / 2 for i in range(5)]
    fid = compute_fid(real, gen, DEV, batch_size=4, weights=weights[1])
    fr = fid_score.extract_features(torch.cat(real), model).cpu().numpy()
    fg = fid_score.extract_features(torch.cat(gen), model).cpu().numpy()
    want = fid_score.calculate_fid(fr, fg)
    assert np.isfinite(fid) and abs(fid - want) <= 1e-6 * abs(want)
