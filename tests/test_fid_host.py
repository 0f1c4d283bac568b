"""The device Fréchet distance without a GPU: the float64 yardstick fid_ref64 against the committed ``calculate_fid`` where
scipy's sqrtm is well-posed, the exported surface of include/dt_hip_fid.h, the workspace query at its limits, the import
surface through the reference's module names, argument checks that fail before any device call, and the default
(``stats`` unset, ``DT_FID_STATS`` unset) staying on the host formula."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from distillation_trajectories_amd import _hip
from fid_ref64 import feature_like, fid_ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", [
    dict(D=64, n_a=300, n_b=257, seed=1),
    dict(D=64, n_a=257, n_b=300, seed=2),
    dict(D=2048, n_a=50, n_b=50, seed=3),
], ids=["D64_300x257", "D64_257x300", "D2048_50x50"])
def test_ref64_agrees_with_the_committed_host_formula(case):
    """|yardstick - calculate_fid| <= 1e-6 (tr S_a + tr S_b): the bound the device is held to in tests/test_hip_fid.py."""
    from distillation_trajectories_amd.analysis.metrics.fid_score import calculate_fid
    a = feature_like(case["seed"], case["n_a"], case["D"])
    b = feature_like(case["seed"] + 100, case["n_b"], case["D"], shift=0.02, spread=0.2)
    ref = fid_ref64(a, b)
    got = calculate_fid(a.astype(np.float64), b.astype(np.float64))
    print(f"{case}: host {got!r} yardstick {ref['fid']!r} deviation / s = {abs(got - ref['fid']) / ref['scale']:.3g}")
    assert abs(got - ref["fid"]) <= 1e-6 * ref["scale"]
    assert ref["parts"][3] > 0 and ref["fid"] > 0


def _fid_header_functions():
    text = open(os.path.join(ROOT, "include", "dt_hip_fid.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_exports_agree():
    from distillation_trajectories_amd.csrc.build import LIB, build
    path = build() if not os.path.exists(LIB) else LIB
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    names = _fid_header_functions()
    assert names == ["dt_fid_distance", "dt_fid_workspace_bytes"]
    assert sorted(_hip.FID_SIGNATURES) == names
    assert set(names) <= exported
    others = (set(_hip.SIGNATURES) | set(_hip.NOISE_SIGNATURES) | set(_hip.INCEPTION_SIGNATURES) |
              set(_hip.PCA_SIGNATURES))
    assert not set(names) & others
    lib = _hip.load(path)
    assert lib.dt_abi_version() == _hip.ABI_VERSION == 6
    assert all(getattr(lib, n).argtypes is not None for n in names)


def test_workspace_query_rejects_shapes_outside_the_limits():
    lib = _hip.load()
    q = lib.dt_fid_workspace_bytes
    for args in ((0, 50, 50, 2048), (65536, 50, 50, 2048), (1, 1, 50, 2048), (1, 50, 1, 2048), (1, 2049, 2049, 2048),
                 (1, 50, 50, 2046), (1, 50, 50, 0), (1, 50, 50, 2), (1, 40000, 50, 2048), (1, -3, 50, 2048)):
        assert q(*args) == 0, args
    # inside: the cross product, the squared matrix and the four D-vectors, and not wildly more
    for P, n_a, n_b, D in ((1, 50, 50, 2048), (11, 8, 50, 2048), (1, 2048, 2048, 2048), (1, 4000, 2048, 64), (3, 2, 2, 4),
                           (65535, 2, 2, 4)):
        m = min(n_a, n_b)
        need = P * (n_a * n_b + m * m + 4 * D) * 8
        got = q(P, n_a, n_b, D)
        assert need < got <= need + P * (8 * m + 64) * 8 + 4 * P + 512, (P, n_a, n_b, D, got, need)


def test_sanitizer_driver_covers_every_fid_entry():
    """tests/host_sanitize/fid_driver.cpp calls every function include/dt_hip_fid.h declares."""
    src = open(os.path.join(ROOT, "tests", "host_sanitize", "fid_driver.cpp")).read()
    missing = [n for n in _fid_header_functions() if n + "(" not in src]
    assert not missing, missing
    from distillation_trajectories_amd.csrc import build
    assert callable(build.build_fid_sanitizer_driver) and "dt_fid.hip" in build.SOURCES
    assert any(h.endswith("dt_hip_fid.h") for h in build.HEADERS)


def test_reference_names_import_after_aliases():
    import distillation_trajectories_amd as pkg
    from distillation_trajectories_amd.analysis.metrics import fid_score as fs
    from distillation_trajectories_amd.evaluation import metrics as em
    pkg.remove_aliases()
    try:
        pkg.install_aliases()
        from analysis.metrics.fid_score import calculate_and_visualize_fid, calculate_fid_device, fid_sweep
        from evaluation.metrics import compute_fid
        assert calculate_fid_device is fs.calculate_fid_device and fid_sweep is fs.fid_sweep
        assert calculate_and_visualize_fid is fs.calculate_and_visualize_fid and compute_fid is em.compute_fid
    finally:
        pkg.remove_aliases()


def test_bad_arguments_raise_before_any_device_call(monkeypatch):
    from distillation_trajectories_amd import engine
    from distillation_trajectories_amd.analysis.metrics import fid_score

    def no_load(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_hip, "load", no_load)
    a = torch.zeros(5, 16)
    with pytest.raises(ValueError, match="float32"):
        engine.device_fid(a.double(), a)
    with pytest.raises(ValueError, match="float32"):
        engine.device_fid(a, a.half())
    with pytest.raises(ValueError, match="torch tensor"):
        engine.device_fid(a.numpy(), a)
    with pytest.raises(ValueError, match=r"\[n, D\] or \[P, n, D\]"):
        engine.device_fid(torch.zeros(16), a)
    with pytest.raises(ValueError, match=r"\[n, D\] or \[P, n, D\]"):
        engine.device_fid(a, torch.zeros(1, 2, 5, 16))
    with pytest.raises(ValueError, match="same feature width"):
        engine.device_fid(a, torch.zeros(5, 20))
    with pytest.raises(ValueError, match="same number of problems"):
        engine.device_fid(torch.zeros(3, 5, 16), torch.zeros(2, 5, 16))
    with pytest.raises(ValueError, match="at least 2 samples"):
        engine.device_fid(a[:1], a)
    with pytest.raises(ValueError, match="at least 2 samples"):
        engine.device_fid(a, torch.zeros(4, 1, 16))
    with pytest.raises(ValueError, match="multiple of 4"):
        engine.device_fid(torch.zeros(5, 18), torch.zeros(5, 18))
    with pytest.raises(ValueError, match="2048.*feature-space"):
        engine.device_fid(torch.zeros(2049, 4), torch.zeros(2049, 4))
    with pytest.raises(ValueError, match="events"):
        engine.device_fid(a, a, events=[None] * 4)
    with pytest.raises(engine.HipLibraryError, match="CUDA"):         # well-formed, but not on the device
        engine.device_fid(a, a)
    for bad in ("gpu", "", 1):
        with pytest.raises(ValueError, match="'host' or 'device'"):
            fid_score.stats_mode(bad)
    with pytest.raises(ValueError, match="num_samples"):
        fid_score.fid_sweep(torch.nn.Linear(1, 1), [torch.nn.Linear(1, 1)], None, 1)
    with pytest.raises(ValueError, match="at least one student"):
        fid_score.fid_sweep(torch.nn.Linear(1, 1), [], None, 5)


def test_placeholder_below_two_samples_without_a_device(monkeypatch, capsys):
    from distillation_trajectories_amd import engine
    from distillation_trajectories_amd.analysis.metrics import fid_score
    monkeypatch.setattr(engine, "device_fid", lambda *a, **k: pytest.fail("device_fid was reached"))
    one, five = np.zeros((1, 8), np.float32), np.zeros((5, 8), np.float32)
    assert fid_score.calculate_fid_device(one, five) == 999.0
    dev_out = capsys.readouterr().out
    assert fid_score.calculate_fid(one, five) == 999.0
    assert dev_out == capsys.readouterr().out and "placeholder FID score of 999.0" in dev_out


class _FakeInception:
    def __init__(self, device, weights=None):
        pass

    def get_features(self, images):
        return feature_like(int(images.sum().item()) % 1000, len(images), 32)


def _host_only_drivers(monkeypatch, tmp_path):
    """both drivers with sampling and the feature network replaced by host stand-ins; returns their results"""
    from distillation_trajectories_amd.analysis.metrics import fid_score
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.evaluation import metrics
    cfg = Config(base_dir=str(tmp_path))
    cfg.num_samples = 6
    calls = iter(range(100))
    monkeypatch.setattr(fid_score, "generate_samples",
                        lambda model, config, n, device, fixed_samples=None: torch.full((n, 3, 4, 4), float(next(calls))))
    monkeypatch.setattr(fid_score, "InceptionModel", _FakeInception)
    monkeypatch.setattr(metrics, "InceptionModel", _FakeInception)
    monkeypatch.setattr(metrics, "extract_features",
                        lambda imgs, model, batch_size=64: torch.from_numpy(feature_like(len(imgs), len(imgs), 32)))
    model = torch.nn.Linear(2, 2)
    res = fid_score.calculate_and_visualize_fid(model, model, cfg, output_dir=str(tmp_path), size_factor=0.5)
    fid = metrics.compute_fid(torch.zeros(7, 3, 4, 4), torch.zeros(5, 3, 4, 4), "cpu")
    return res, fid


def test_default_never_reaches_the_device_path(monkeypatch, tmp_path):
    from distillation_trajectories_amd import engine
    from distillation_trajectories_amd.analysis.metrics import fid_score

    def no_device(*a, **k):
        raise AssertionError("device_fid was reached with stats unset")
    monkeypatch.delenv("DT_FID_STATS", raising=False)
    monkeypatch.setattr(engine, "device_fid", no_device)
    assert fid_score.stats_mode() == "host" and fid_score.stats_mode(None) == "host"
    res, fid = _host_only_drivers(monkeypatch, tmp_path)
    want = fid_score.calculate_fid(feature_like(0, 6, 32), feature_like(6 * 48 % 1000, 6, 32))
    assert res == {"fid_score": want}
    assert fid == pytest.approx(fid_score.calculate_fid(feature_like(7, 7, 32), feature_like(5, 5, 32)), rel=1e-6)
    with open(tmp_path / "fid_score_size_0.5.txt") as f:
        assert f.read() == f"FID Score: {want:.4f}\n"


def test_environment_switch_supplies_the_default(monkeypatch, tmp_path):
    from distillation_trajectories_amd import engine
    from distillation_trajectories_amd.analysis.metrics import fid_score
    from distillation_trajectories_amd.evaluation import metrics

    class Reached(Exception):
        pass

    def device(*a, **k):
        raise Reached
    monkeypatch.setattr(engine, "device_fid", device)
    monkeypatch.setenv("DT_FID_STATS", "device")
    assert fid_score.stats_mode() == "device" and fid_score.stats_mode("host") == "host"
    monkeypatch.setattr(metrics, "InceptionModel", _FakeInception)
    monkeypatch.setattr(metrics, "extract_features",
                        lambda imgs, model, batch_size=64: torch.from_numpy(feature_like(len(imgs), len(imgs), 32)))
    assert np.isfinite(metrics.compute_fid(torch.zeros(7, 3, 4, 4), torch.zeros(5, 3, 4, 4), "cpu", stats="host"))
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)      # no device to upload to here
    with pytest.raises(Reached):
        metrics.compute_fid(torch.zeros(7, 3, 4, 4), torch.zeros(5, 3, 4, 4), "cpu")
    monkeypatch.setenv("DT_FID_STATS", "host")
    assert np.isfinite(metrics.compute_fid(torch.zeros(7, 3, 4, 4), torch.zeros(5, 3, 4, 4), "cpu"))
    monkeypatch.setenv("DT_FID_STATS", "both")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        metrics.compute_fid(torch.zeros(7, 3, 4, 4), torch.zeros(5, 3, 4, 4), "cpu")
