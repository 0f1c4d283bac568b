"""The InceptionV3 feature extractor without a GPU: the C ABI of include/dt_hip_inception.h against the binding, the
library's exports, its own layer table and the sanitizer driver; torchvision's key table and the state-dict loader;
the resize contract; input checks and the missing-weights error (tests/test_hip_inception.py runs it on the GPU)."""
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from distillation_trajectories_amd import _hip, inception

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    text = open(os.path.join(ROOT, "include", "dt_hip_inception.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


def _lib_path():
    from distillation_trajectories_amd.csrc.build import LIB, build
    return build() if not os.path.exists(LIB) else LIB


def test_header_binding_and_exports_agree():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    names = _header_functions()
    assert len(names) == 8
    assert sorted(_hip.INCEPTION_SIGNATURES) == names
    assert set(names) <= exported
    lib = _hip.load(_lib_path())
    assert lib.dt_abi_version() == _hip.ABI_VERSION == 6
    assert all(getattr(lib, n).argtypes is not None for n in names)
    assert not set(names) & (set(_hip.SIGNATURES) | set(_hip.NOISE_SIGNATURES))


def test_sanitizer_driver_covers_every_inception_entry():
    src = open(os.path.join(ROOT, "tests", "host_sanitize", "inception_driver.cpp")).read()
    missing = [n for n in _header_functions() if n + "(" not in src]
    assert not missing, missing


def test_library_layer_table_matches_torchvision_table():
    """The library's conv table (dt_inception_conv_desc) is the Python table, conv for conv, and its module shapes chain."""
    _hip.load(_lib_path())
    assert len(inception.CONVS) == 94 and len(inception.MODULES) == 19
    for i, (name, *desc) in enumerate(inception.CONVS):
        assert inception.conv_desc(i) == tuple(desc), name
    prev = (299, 299, 3)
    for m, name in enumerate(inception.MODULES):
        shape_in, shape_out = inception.module_shape(m)
        assert shape_in == prev, name
        prev = shape_out
    assert prev == (1, 1, 2048)
    assert inception.module_shape(10)[1] == (17, 17, 768) and inception.module_shape(15)[1] == (8, 8, 1280)


def test_key_table_parameter_count():
    """torchvision's num_params of Inception_V3_Weights.IMAGENET1K_V1 (AuxLogits and fc included, running stats not)."""
    assert inception.parameter_count() == 27_161_264
    table = inception.key_table()
    assert table["Mixed_6b.branch7x7_2.conv.weight"] == (128, 128, 1, 7)
    assert table["Mixed_7c.branch_pool.conv.weight"] == (192, 2048, 1, 1)
    assert table["AuxLogits.conv1.conv.weight"] == (768, 128, 5, 5)
    assert len(inception.required_keys()) == 5 * 94


@pytest.fixture(scope="module")
def full_state_dict():
    g = torch.Generator().manual_seed(3)
    sd = {}
    for k, shape in inception.key_table().items():
        sd[k] = torch.randn(shape, generator=g)
        if k.endswith("running_var"):
            sd[k] = sd[k].abs() + 0.5
            sd[k[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(7)
    return sd


def test_loader_accepts_full_torchvision_state_dict(full_state_dict):
    tensors = inception.check_state_dict(full_state_dict)
    assert len(tensors) == 470
    assert tensors[0] is full_state_dict["Conv2d_1a_3x3.conv.weight"]
    assert tensors[-1] is full_state_dict["Mixed_7c.branch_pool.bn.running_var"]
    no_aux = {k: v for k, v in full_state_dict.items() if not k.startswith(("AuxLogits.", "fc."))}
    assert len(inception.check_state_dict(no_aux)) == 470


def test_loader_rejects_missing_and_misshaped_keys(full_state_dict):
    sd = dict(full_state_dict)
    del sd["Mixed_6c.branch7x7dbl_4.bn.running_mean"]
    with pytest.raises(ValueError, match=re.escape("Mixed_6c.branch7x7dbl_4.bn.running_mean")):
        inception.check_state_dict(sd)
    sd = dict(full_state_dict)
    k = "Mixed_6b.branch7x7_2.conv.weight"             # 1x7 given as 7x1
    sd[k] = sd[k].transpose(2, 3).contiguous()
    with pytest.raises(ValueError, match=re.escape(k)):
        inception.check_state_dict(sd)
    sd = dict(full_state_dict)
    sd["Mixed_5b.branch9x9.conv.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="Mixed_5b.branch9x9"):
        inception.check_state_dict(sd)


@pytest.mark.parametrize("size", [16, 32, 64])
def test_upsampling_resize_is_the_same_with_and_without_antialias(size):
    """torchvision's Resize antialias default only matters when downsampling: pinned in float64 for size -> 299."""
    x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(size), dtype=torch.float64)
    a = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False, antialias=True)
    b = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False, antialias=False)
    assert (a - b).abs().max().item() <= 1e-12


def test_bad_images_raise_before_any_device_call():
    from distillation_trajectories_amd.analysis.metrics.fid_score import extract_features
    with pytest.raises(ValueError, match="3 channels"):
        extract_features(torch.zeros(2, 1, 16, 16))
    with pytest.raises(ValueError, match="300x16"):
        extract_features(torch.zeros(2, 3, 300, 16))
    with pytest.raises(ValueError, match="16x300"):
        extract_features(torch.zeros(2, 3, 16, 300))
    with pytest.raises(ValueError, match="no images"):
        extract_features(torch.zeros(0, 3, 16, 16))
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        extract_features(torch.zeros(3, 16, 16))


def test_missing_weights_name_the_variable(monkeypatch):
    from distillation_trajectories_amd.analysis.metrics.fid_score import InceptionModel, extract_features
    monkeypatch.delenv(inception.WEIGHTS_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match="DT_INCEPTION_WEIGHTS") as e:
        InceptionModel("cuda")
    assert "inception_v3_google-0cc3c7bd.pth" in str(e.value)
    with pytest.raises(FileNotFoundError, match="DT_INCEPTION_WEIGHTS"):
        extract_features(torch.zeros(1, 3, 8, 8))
    monkeypatch.setenv(inception.WEIGHTS_ENV, os.path.join(ROOT, "no_such_weights.pth"))
    with pytest.raises(FileNotFoundError, match="no_such_weights.pth"):
        InceptionModel("cuda")


def test_weights_file_loads_with_weights_only(tmp_path, full_state_dict):
    path = tmp_path / "w.pth"
    torch.save(full_state_dict, path)
    sd = inception.read_weights(str(path))
    assert torch.equal(sd["fc.weight"], full_state_dict["fc.weight"])


def test_reference_names_import_after_aliases():
    import distillation_trajectories_amd as pkg
    pkg.remove_aliases()
    try:
        pkg.install_aliases()
        from analysis.metrics.fid_score import InceptionModel, calculate_and_visualize_fid, extract_features
        from evaluation.metrics import compute_fid
        assert all(callable(f) for f in (InceptionModel, calculate_and_visualize_fid, extract_features, compute_fid))
    finally:
        pkg.remove_aliases()
