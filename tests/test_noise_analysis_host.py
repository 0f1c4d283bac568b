"""The noise-prediction driver and sweep without a GPU: import surface through the reference's module names, the exported
dt_q_sample, the timestep list and fp32 noising coefficients, and the txt formatter -- against the reference's own run
(tests/golden/make_golden_noise.py)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from distillation_trajectories_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


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


def test_reference_names_import_after_aliases():
    import distillation_trajectories_amd as pkg
    pkg.remove_aliases()
    try:
        pkg.install_aliases()
        from analysis.noise_prediction.noise_analysis import analyze_noise_prediction, noise_prediction_sweep
        assert callable(analyze_noise_prediction) and callable(noise_prediction_sweep)
    finally:
        pkg.remove_aliases()


def _noise_header_functions():
    text = open(os.path.join(ROOT, "include", "dt_hip_noise.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_q_sample():
    from distillation_trajectories_amd.csrc.build import LIB, build
    path = build() if not os.path.exists(LIB) else LIB
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    assert _noise_header_functions() == ["dt_q_sample"]
    assert sorted(_hip.NOISE_SIGNATURES) == _noise_header_functions()
    assert set(_hip.NOISE_SIGNATURES) <= exported
    lib = _hip.load(path)
    assert lib.dt_abi_version() == _hip.ABI_VERSION == 6
    assert lib.dt_q_sample.argtypes is not None


def test_noise_sanitizer_driver_covers_every_noise_entry():
    """tests/host_sanitize/noise_driver.cpp calls every function include/dt_hip_noise.h declares."""
    src = open(os.path.join(ROOT, "tests", "host_sanitize", "noise_driver.cpp")).read()
    missing = [n for n in _noise_header_functions() if n + "(" not in src]
    assert not missing, missing


def test_timesteps_and_coefficients_bit_identical(golden_noise):
    from distillation_trajectories_amd.analysis.noise_prediction.noise_analysis import N_TIMESTEPS, noise_coefficients
    arrays, meta = golden_noise
    t_list = torch.linspace(0, meta["T"] - 1, N_TIMESTEPS, dtype=torch.long).tolist()
    assert t_list == meta["timesteps"]
    coef = noise_coefficients(_config(meta["T"]), t_list)
    assert coef.dtype == torch.float32
    assert np.array_equal(coef.numpy().view(np.uint32), arrays["coef"].view(np.uint32))


def test_coefficients_of_any_subset_match_the_full_table():
    """The running product gives every t the reference's own product, whichever timesteps are asked for together."""
    from distillation_trajectories_amd.analysis.noise_prediction.noise_analysis import noise_coefficients
    c = _config(50)
    full = noise_coefficients(c, range(50))
    for sub in ([49], [0, 7, 31], [12, 3]):
        assert torch.equal(noise_coefficients(c, sub), full[sub])


def test_txt_formatter_byte_identical(golden_noise):
    from distillation_trajectories_amd.analysis.noise_prediction.noise_analysis import format_noise_metrics
    _, meta = golden_noise
    for case in meta["cases"].values():
        res = {"avg_mse": np.float64(case["avg_mse"]), "avg_mae": np.float64(case["avg_mae"]),
               "avg_cosine_similarity": np.float64(case["avg_cosine_similarity"]),
               "metrics_by_timestep": {int(t): m for t, m in case["metrics_by_timestep"].items()}}
        assert format_noise_metrics(res) == case["txt"]


def test_driver_without_images_names_fixed_samples():
    from distillation_trajectories_amd.analysis.noise_prediction.noise_analysis import _dataset_images
    with pytest.raises(ValueError, match="fixed_samples"):
        _dataset_images(object(), torch.device("cpu"))
