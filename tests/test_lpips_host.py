"""LPIPS without a GPU: the C ABI of include/dt_hip_lpips.h against the binding and the library's exports, the key table
and both weight layouts, loader and input errors, the missing-weights error, and the float64 / float32 restatement
(tests/lpips_ref64.py) whose own fp32 error is the yardstick of the device's distance bounds
(tests/test_hip_lpips.py runs the device side)."""
import os
import re
import subprocess

import pytest
import torch

import lpips_ref64 as ref
from distillation_trajectories_amd import _hip, lpips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The fp32 restatement's maximum relative error against float64 on the committed inputs (ref.pair_inputs over ref.SIZES,
# weights ref.random_state_dict(11)), measured with torch-CPU: (total, per layer).  tests/test_hip_lpips.py bounds the
# device by 4 x these.
YARDSTICK = {"independent": (1.78e-7, 1.04e-6), "near": (2.59e-6, 1.14e-5)}


def _header_functions():
    text = open(os.path.join(ROOT, "include", "dt_hip_lpips.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


def _lib_path():
    from distillation_trajectories_amd.csrc.build import LIB, build
    return build() if not os.path.exists(LIB) else LIB


def test_header_binding_and_exports_agree():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    names = _header_functions()
    assert len(names) == 9
    assert sorted(_hip.LPIPS_SIGNATURES) == names
    assert set(names) <= exported
    lib = _hip.load(_lib_path())
    assert lib.dt_abi_version() == _hip.ABI_VERSION
    others = (set(_hip.SIGNATURES) | set(_hip.NOISE_SIGNATURES) | set(_hip.INCEPTION_SIGNATURES) |
              set(_hip.PCA_SIGNATURES) | set(_hip.FID_SIGNATURES))
    assert not set(names) & others


def test_build_lists_the_source_header_and_driver():
    from distillation_trajectories_amd.csrc import build
    assert "dt_lpips.hip" in build.SOURCES and any(h.endswith("dt_hip_lpips.h") for h in build.HEADERS)
    assert callable(build.build_lpips_sanitizer_driver)
    src = open(os.path.join(ROOT, "tests", "host_sanitize", "lpips_driver.cpp")).read()
    missing = [n for n in _header_functions() if n + "(" not in src]
    assert not missing, missing


def test_library_shapes_match_the_python_table_and_the_restatement():
    """dt_lpips_layer_shape / dt_lpips_feature_floats (host code: no device call) against lpips.layer_shapes and against
    the shapes the torch restatement produces; sizes outside 31..299 give a negative status / 0."""
    lib = _hip.load(_lib_path())
    sd = ref.random_state_dict(1)
    for H, W in ((31, 31), (32, 32), (35, 47), (64, 64), (299, 31), (299, 299)):
        shapes = lpips.layer_shapes(H, W)
        assert [lpips.layer_shape(H, W, l) for l in range(5)] == shapes
        assert lpips.feature_floats(H, W) == sum(h * w * c for h, w, c in shapes)
        if H * W <= 64 * 64:
            got = [(t.shape[2], t.shape[3], t.shape[1]) for t in ref.taps(sd, ref.images(1, H, W, seed=0))]
            assert got == shapes
    assert lpips.layer_shapes(31, 31)[2:] == [(1, 1, 384), (1, 1, 256), (1, 1, 256)]
    assert lpips.layer_shapes(64, 64)[2] == (3, 3, 384)
    import ctypes
    d = (ctypes.c_int * 3)()
    for H, W in ((30, 30), (31, 30), (300, 64), (64, 300), (0, 0)):
        assert lib.dt_lpips_layer_shape(H, W, 0, d) == -2
        assert lib.dt_lpips_feature_floats(H, W) == 0
        assert lib.dt_lpips_workspace_bytes(None, 1, H, W) == 0
    assert lib.dt_lpips_layer_shape(32, 32, 5, d) == -3 and lib.dt_lpips_layer_shape(32, 32, -1, d) == -3
    assert lib.dt_lpips_layer_shape(32, 32, 0, None) == -1


def test_key_table_names_both_layouts():
    t = lpips.key_table("lpips")
    assert t["net.slice1.0.weight"] == (64, 3, 11, 11) and t["net.slice1.0.bias"] == (64,)
    assert t["net.slice2.3.weight"] == (192, 64, 5, 5) and t["net.slice3.6.weight"] == (384, 192, 3, 3)
    assert t["net.slice4.8.weight"] == (256, 384, 3, 3) and t["net.slice5.10.weight"] == (256, 256, 3, 3)
    assert t["lin0.model.1.weight"] == (1, 64, 1, 1) and t["lins.4.model.1.weight"] == (1, 256, 1, 1)
    tv = lpips.key_table("torchvision")
    assert sorted(tv) == sorted(f"features.{i}.{leaf}" for i in (0, 3, 6, 8, 10) for leaf in ("weight", "bias"))
    assert sorted(lpips.key_table("lins")) == sorted([f"lin{k}.model.1.weight" for k in range(5)] +
                                                     [f"lins.{k}.model.1.weight" for k in range(5)])
    assert lpips.CHANNELS == (64, 192, 384, 256, 256)


def _pair(sd):
    """layout (b) from a layout (a) state dict: torchvision AlexNet (classifier included) and alex.pth"""
    names = {"net.slice1.0": "features.0", "net.slice2.3": "features.3", "net.slice3.6": "features.6",
             "net.slice4.8": "features.8", "net.slice5.10": "features.10"}
    tv = {f"{names[k.rsplit('.', 1)[0]]}.{k.rsplit('.', 1)[1]}": v for k, v in sd.items() if k.startswith("net.")}
    tv["classifier.1.weight"], tv["classifier.6.bias"] = torch.zeros(4096, 9216), torch.zeros(1000)
    lins = {k: v for k, v in sd.items() if k.startswith("lin")}
    return tv, lins


def test_loader_accepts_both_layouts_in_create_order():
    sd = ref.random_state_dict(2, torch.float32)
    tensors = lpips.check_state_dict(sd)
    assert len(tensors) == 15
    assert tensors[0] is sd["net.slice1.0.weight"] and tensors[1] is sd["net.slice1.0.bias"]
    assert tensors[8] is sd["net.slice5.10.weight"] and tensors[10] is sd["lin0.model.1.weight"]
    assert tensors[14] is sd["lin4.model.1.weight"]
    tv, lins = _pair(sd)
    again = lpips.check_state_dict((tv, lins))
    assert len(again) == 15 and all(a is b for a, b in zip(tensors, again))
    # the ModuleList names of the same lin tensors, alone or next to the attribute names
    alias = {k: v for k, v in sd.items() if not k.startswith("lin")}
    alias.update({f"lins.{k}.model.1.weight": sd[f"lin{k}.model.1.weight"] for k in range(5)})
    assert all(a is b for a, b in zip(tensors, lpips.check_state_dict(alias)))
    assert all(a is b for a, b in zip(tensors, lpips.check_state_dict({**sd, **alias})))


def test_loader_errors_name_the_key():
    sd = ref.random_state_dict(2, torch.float32)
    bad = dict(sd)
    del bad["net.slice3.6.bias"]
    with pytest.raises(ValueError, match=re.escape("net.slice3.6.bias")):
        lpips.check_state_dict(bad)
    bad = dict(sd)
    del bad["lin3.model.1.weight"]
    with pytest.raises(ValueError, match=re.escape("lin3.model.1.weight")):
        lpips.check_state_dict(bad)
    bad = dict(sd)
    bad["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=re.escape("net.slice2.3.weight")):
        lpips.check_state_dict(bad)
    bad = dict(sd)
    bad["net.slice6.12.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match=re.escape("net.slice6.12.weight")):
        lpips.check_state_dict(bad)
    tv, lins = _pair(sd)
    with pytest.raises(ValueError, match=re.escape("features.8.weight")):
        lpips.check_state_dict(({k: v for k, v in tv.items() if k != "features.8.weight"}, lins))
    with pytest.raises(ValueError, match=re.escape("lin0.model.1.weight")):
        lpips.check_state_dict((tv, {k: v for k, v in lins.items() if k != "lin0.model.1.weight"}))
    with pytest.raises(ValueError, match=re.escape("lin1.model.1.weight")):
        lpips.check_state_dict((tv, {**lins, "lin1.model.1.weight": torch.zeros(1, 64, 1, 1)}))
    with pytest.raises(ValueError, match=re.escape("features.1.weight")):
        lpips.check_state_dict(({**tv, "features.1.weight": torch.zeros(1)}, lins))
    with pytest.raises(ValueError, match="2 members"):
        lpips.check_state_dict((tv, lins, lins))


def test_read_weights_paths_pairs_and_the_variable(tmp_path, monkeypatch):
    sd = ref.random_state_dict(3, torch.float32)
    tv, lins = _pair(sd)
    one, alexnet, alex = tmp_path / "lpips_alex.pth", tmp_path / "alexnet.pth", tmp_path / "alex.pth"
    torch.save(sd, one), torch.save(tv, alexnet), torch.save(lins, alex)
    want = lpips.check_state_dict(sd)

    def same(weights):
        return all(torch.equal(a, b) for a, b in zip(want, lpips.check_state_dict(lpips.read_weights(weights))))

    assert same(str(one)) and same(sd) and same((tv, lins)) and same((str(alexnet), str(alex)))
    assert same(f"{alexnet},{alex}")
    monkeypatch.setenv(lpips.WEIGHTS_ENV, str(one))
    assert same(None)
    monkeypatch.setenv(lpips.WEIGHTS_ENV, f"{alexnet},{alex}")
    assert same(None)
    monkeypatch.setenv(lpips.WEIGHTS_ENV, str(tmp_path / "no_such_weights.pth"))
    with pytest.raises(FileNotFoundError, match="no_such_weights.pth"):
        lpips.read_weights()


def test_missing_weights_name_the_variable_and_give_no_placeholder(monkeypatch):
    from distillation_trajectories_amd.evaluation.metrics import LPIPSModel, compute_lpips
    from distillation_trajectories_amd.analysis.metrics.perceptual import lpips_sweep
    from distillation_trajectories_amd.config import Config
    monkeypatch.delenv(lpips.WEIGHTS_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match="DT_LPIPS_WEIGHTS"):
        LPIPSModel("cuda")
    with pytest.raises(FileNotFoundError, match="DT_LPIPS_WEIGHTS"):
        compute_lpips(torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 32), "cuda")
    cfg = Config()
    cfg.image_size, cfg.timesteps = 32, 4
    teacher = torch.nn.Linear(1, 1)
    with pytest.raises(FileNotFoundError, match="DT_LPIPS_WEIGHTS"):
        lpips_sweep(teacher, [teacher], cfg, [1.0], 2)


def test_compute_lpips_takes_one_image_per_argument():
    from distillation_trajectories_amd.evaluation.metrics import compute_lpips
    sd = ref.random_state_dict(2, torch.float32)
    with pytest.raises(ValueError, match="lpips_distances"):
        compute_lpips(torch.rand(2, 3, 32, 32), torch.rand(2, 3, 32, 32), "cuda", weights=sd)
    with pytest.raises(ValueError, match="lpips_distances"):
        compute_lpips(torch.rand(1, 3, 32, 32), torch.rand(2, 3, 32, 32), "cuda", weights=sd)
    with pytest.raises(ValueError, match="30x30"):
        compute_lpips(torch.rand(1, 3, 30, 30), torch.rand(1, 3, 30, 30), "cuda", weights=sd)
    with pytest.raises(ValueError, match="3 channels"):
        compute_lpips(torch.rand(1, 1, 32, 32), torch.rand(1, 1, 32, 32), "cuda", weights=sd)


def test_lpips_sweep_rejects_small_images_before_sampling():
    from distillation_trajectories_amd.analysis.metrics.perceptual import lpips_sweep, state_indices
    from distillation_trajectories_amd.config import Config
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 4

    class NoSampling(torch.nn.Module):
        def parameters(self, recurse=True):
            raise AssertionError("the model was touched before the size check")

    with pytest.raises(ValueError, match="16x16"):
        lpips_sweep(NoSampling(), [NoSampling()], cfg, [1.0, 3.0], 2, weights={})
    with pytest.raises(ValueError, match="30x64"):
        lpips_sweep(NoSampling(), [NoSampling()], cfg, [1.0], 2, weights={}, resize=(30, 64))
    assert state_indices(5, 1) == [0, 1, 2, 3, 4] and state_indices(5, 2) == [0, 2, 4] and state_indices(6, 4) == [0, 4, 5]


def test_reference_names_import_after_aliases():
    import distillation_trajectories_amd as pkg
    pkg.remove_aliases()
    try:
        pkg.install_aliases()
        from evaluation.metrics import LPIPSModel, compute_lpips, lpips_distances
        assert all(callable(f) for f in (LPIPSModel, compute_lpips, lpips_distances))
    finally:
        pkg.remove_aliases()


def test_restatement_rejects_30x30_and_has_live_layers():
    sd = ref.random_state_dict(11)
    with pytest.raises(RuntimeError):
        ref.taps(sd, ref.images(1, 30, 30, seed=1))
    for hw in ref.SIZES:
        for t in ref.taps(sd, ref.images(4, *hw, seed=3)):
            assert (t != 0).double().mean().item() > 0.3


def test_restatement_properties_in_float64():
    sd = ref.random_state_dict(11)
    a, b = ref.pair_inputs((32, 32), "independent", n=3)
    d_ab, l_ab = ref.distance(sd, a, b)
    d_ba, _ = ref.distance(sd, b, a)
    assert torch.equal(d_ab, d_ba) and torch.equal(ref.distance(sd, a, a)[0], torch.zeros(3, dtype=torch.float64))
    assert torch.allclose(l_ab.sum(dim=1), d_ab, rtol=1e-14) and (l_ab > 0).all()
    shared, _ = ref.distance(sd, a[:1], b)
    assert torch.equal(shared[0], d_ab[0])
    # the (2, -1) map of [0, 1] images is the (1, 0) map of 2x - 1
    u = (a + 1) / 2
    assert torch.allclose(ref.distance(sd, u.double(), ((b + 1) / 2).double(), 2.0, -1.0)[0], d_ab, rtol=1e-9)


@pytest.mark.parametrize("kind", ["independent", "near"])
def test_fp32_restatement_against_float64_is_the_recorded_yardstick(kind):
    """The fp32 evaluation of the restatement (what the lpips package computes) against float64 on the device test's
    inputs.  The recorded maxima set the device's bounds; another CPU sums in another order, so the measurement has to
    agree with the record only within the factor that two fp32 summation orders differ by."""
    sd32 = ref.random_state_dict(11, torch.float32)
    total, per_layer = ref.yardstick(sd32, kind)
    print(f"yardstick {kind}: total {total:.3g}, per layer {per_layer:.3g} (recorded {YARDSTICK[kind]})")
    rec_total, rec_layer = YARDSTICK[kind]
    assert rec_total / 4 <= total <= rec_total * 4
    assert rec_layer / 4 <= per_layer <= rec_layer * 4
    sd64 = ref.cast(sd32, torch.float64)
    d = torch.cat([ref.distance(sd64, *ref.pair_inputs(hw, kind))[0] for hw in ref.SIZES])
    assert (0.5 < d.min() and d.max() < 1.5) if kind == "independent" else (1e-3 < d.min() and d.max() < 1e-2)
