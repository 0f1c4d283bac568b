"""InceptionV3 features for FID on libdt_hip (include/dt_hip_inception.h).

The network is torchvision's ``Inception3`` in eval mode with ``transform_input=False`` and ``fc = Identity``: the
2048 ``avgpool`` values per image that the reference's ``InceptionModel.get_features`` and ``compute_fid`` use.  Weights
are the user's own copy of torchvision's ``inception_v3_google-0cc3c7bd.pth`` (a plain state dict), given as a path or a
state dict, or named by ``DT_INCEPTION_WEIGHTS``; nothing is ever downloaded.

This module holds the torchvision key table, the state-dict loader that checks a state dict against it, and
``InceptionHandle``, the device handle (BatchNorm is folded on the device at create time).
"""
import os
from ctypes import c_int

import torch

from . import _hip
from ._hip import check, ptr, stream_ptr

WEIGHTS_ENV = "DT_INCEPTION_WEIGHTS"
WEIGHTS_FILE = "inception_v3_google-0cc3c7bd.pth"
SIZE = 299
N_FEATURES = 2048
BN_EPS = 1e-3


def _network():
    """(convs, modules): every BasicConv2d as (name, cin, cout, kh, kw, stride, pad_h, pad_w) in forward order, which
    is torchvision's module order and the order dt_inception_create takes them in, and the 19 module names of the
    module-range entry (include/dt_hip_inception.h)."""
    convs, modules = [], []

    def c(name, cin, cout, kh, kw, stride=1, ph=0, pw=0):
        convs.append((name, cin, cout, kh, kw, stride, ph, pw))

    c("Conv2d_1a_3x3", 3, 32, 3, 3, 2)
    c("Conv2d_2a_3x3", 32, 32, 3, 3)
    c("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1)
    c("Conv2d_3b_1x1", 64, 80, 1, 1)
    c("Conv2d_4a_3x3", 80, 192, 3, 3)
    modules += ["Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxpool1", "Conv2d_3b_1x1", "Conv2d_4a_3x3",
                "maxpool2"]
    for name, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):     # InceptionA
        c(f"{name}.branch1x1", cin, 64, 1, 1)
        c(f"{name}.branch5x5_1", cin, 48, 1, 1)
        c(f"{name}.branch5x5_2", 48, 64, 5, 5, 1, 2, 2)
        c(f"{name}.branch3x3dbl_1", cin, 64, 1, 1)
        c(f"{name}.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1)
        c(f"{name}.branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1)
        c(f"{name}.branch_pool", cin, pf, 1, 1)
        modules.append(name)
    c("Mixed_6a.branch3x3", 288, 384, 3, 3, 2)                                                      # InceptionB
    c("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1)
    c("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1)
    c("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3, 2)
    modules.append("Mixed_6a")
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):     # InceptionC
        c(f"{name}.branch1x1", 768, 192, 1, 1)
        c(f"{name}.branch7x7_1", 768, c7, 1, 1)
        c(f"{name}.branch7x7_2", c7, c7, 1, 7, 1, 0, 3)
        c(f"{name}.branch7x7_3", c7, 192, 7, 1, 1, 3, 0)
        c(f"{name}.branch7x7dbl_1", 768, c7, 1, 1)
        c(f"{name}.branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0)
        c(f"{name}.branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3)
        c(f"{name}.branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0)
        c(f"{name}.branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3)
        c(f"{name}.branch_pool", 768, 192, 1, 1)
        modules.append(name)
    c("Mixed_7a.branch3x3_1", 768, 192, 1, 1)                                                       # InceptionD
    c("Mixed_7a.branch3x3_2", 192, 320, 3, 3, 2)
    c("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1)
    c("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3)
    c("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0)
    c("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3, 2)
    modules.append("Mixed_7a")
    for name, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):                                      # InceptionE
        c(f"{name}.branch1x1", cin, 320, 1, 1)
        c(f"{name}.branch3x3_1", cin, 384, 1, 1)
        c(f"{name}.branch3x3_2a", 384, 384, 1, 3, 1, 0, 1)
        c(f"{name}.branch3x3_2b", 384, 384, 3, 1, 1, 1, 0)
        c(f"{name}.branch3x3dbl_1", cin, 448, 1, 1)
        c(f"{name}.branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1)
        c(f"{name}.branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1)
        c(f"{name}.branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0)
        c(f"{name}.branch_pool", cin, 192, 1, 1)
        modules.append(name)
    modules.append("avgpool")
    return convs, modules


CONVS, MODULES = _network()
BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def _basic_keys(name, cin, cout, kh, kw):
    return [(f"{name}.conv.weight", (cout, cin, kh, kw))] + [(f"{name}.bn.{k}", (cout,)) for k in BN_KEYS]


def key_table():
    """{key: shape} of torchvision's Inception3 state dict (num_batches_tracked omitted), AuxLogits and fc included."""
    rows = []
    for name, cin, cout, kh, kw, *_ in CONVS:
        rows += _basic_keys(name, cin, cout, kh, kw)
    rows += _basic_keys("AuxLogits.conv0", 768, 128, 1, 1) + _basic_keys("AuxLogits.conv1", 128, 768, 5, 5)
    rows += [("AuxLogits.fc.weight", (1000, 768)), ("AuxLogits.fc.bias", (1000,)),
             ("fc.weight", (1000, 2048)), ("fc.bias", (1000,))]
    return dict(rows)


def required_keys():
    """The keys the feature extractor uses, in dt_inception_create's order (five per BasicConv2d)."""
    return [k for name, cin, cout, kh, kw, *_ in CONVS for k, _ in _basic_keys(name, cin, cout, kh, kw)]


def parameter_count():
    """Learnable parameters of the key table (conv weights, BatchNorm weight / bias, fc weight / bias)."""
    n = 0
    for k, shape in key_table().items():
        if not k.endswith(("running_mean", "running_var")):
            p = 1
            for s in shape:
                p *= s
            n += p
    return n


def _ignored(key):
    return key.endswith("num_batches_tracked") or key.startswith(("AuxLogits.", "fc."))


def check_state_dict(state_dict):
    """The 470 tensors the extractor uses, in dt_inception_create's order, from a torchvision-layout state dict.
    AuxLogits.*, fc.* and num_batches_tracked are accepted and ignored; a missing, mis-shaped or unknown key raises
    ValueError naming it."""
    table = key_table()
    for k, v in state_dict.items():
        if k not in table and not _ignored(k):
            raise ValueError(f"InceptionV3 state dict: unexpected key '{k}'")
        if k in table and tuple(v.shape) != table[k]:
            raise ValueError(f"InceptionV3 state dict: '{k}' has shape {tuple(v.shape)}, expected {table[k]}")
    out = []
    for k in required_keys():
        if k not in state_dict:
            raise ValueError(f"InceptionV3 state dict: missing key '{k}'")
        out.append(state_dict[k])
    return out


def read_weights(weights=None):
    """A state dict from ``weights`` (a path or a mapping) or from the file ``$DT_INCEPTION_WEIGHTS`` names."""
    if weights is None:
        weights = os.environ.get(WEIGHTS_ENV) or None
    if weights is None:
        raise FileNotFoundError(
            f"no InceptionV3 weights: pass weights=<path or state dict> or set {WEIGHTS_ENV} to a copy of torchvision's "
            f"{WEIGHTS_FILE} (the IMAGENET1K_V1 state dict). Weights are never downloaded.")
    if isinstance(weights, (str, os.PathLike)):
        if not os.path.exists(weights):
            raise FileNotFoundError(f"InceptionV3 weights file {weights} does not exist (expected torchvision's "
                                    f"{WEIGHTS_FILE})")
        weights = torch.load(weights, map_location="cpu", weights_only=True)
    return weights


def check_images(images):
    """Raise ValueError unless ``images`` is an [N, 3, H, W] tensor with N >= 1 and 1 <= H, W <= 299."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError(f"InceptionV3 features: images must be an [N, 3, H, W] tensor, got "
                         f"{tuple(images.shape) if isinstance(images, torch.Tensor) else type(images).__name__}")
    N, C, H, W = images.shape
    if C != 3:
        raise ValueError(f"InceptionV3 features: images must have 3 channels, got {C}")
    if not (1 <= H <= SIZE and 1 <= W <= SIZE):
        raise ValueError(f"InceptionV3 features: image size {H}x{W} is outside 1..{SIZE} (inputs are upsampled to "
                         f"{SIZE}x{SIZE}; downsampling is not supported)")
    if N < 1:
        raise ValueError("InceptionV3 features: no images")


def conv_desc(i):
    """(cin, cout, kh, kw, stride, pad_h, pad_w) of BasicConv2d i as the library's table has it."""
    d = (c_int * 7)()
    check(_hip.load().dt_inception_conv_desc(i, d), "dt_inception_conv_desc")
    return tuple(d)


def module_shape(m):
    """((H, W, C) in, (H, W, C) out) of module m as the library's table has it."""
    a, b = (c_int * 3)(), (c_int * 3)()
    check(_hip.load().dt_inception_module_shape(m, a, b), "dt_inception_module_shape")
    return tuple(a), tuple(b)


class InceptionHandle(_hip.DeviceHandle):
    """The network's weights on one device (dt_inception_create) and a workspace grown on demand: ``workspace(B)``."""
    ENTRY, GPU_ONLY = "dt_inception", "InceptionV3 features run"

    def __init__(self, state_dict, device):
        super().__init__(check_state_dict(state_dict), device)

    def _images(self, images):
        check_images(images)
        return images.detach().to(self.device, torch.float32).contiguous()

    def preprocess(self, images, in_scale=1.0, in_shift=0.0):
        """[N, 299, 299, 3] NHWC: the input of module 0 (dt_inception_preprocess)."""
        x = self._images(images)
        N, C, H, W = x.shape
        out = torch.empty(N, SIZE, SIZE, 3, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(_hip.load().dt_inception_preprocess(ptr(x), N, C, H, W, in_scale, in_shift, ptr(out), stream_ptr()),
                  "dt_inception_preprocess")
        return out

    def features(self, images, in_scale=1.0, in_shift=0.0, out=None):
        """[N, 2048] fp32 on the device for images [N, 3, H, W] (one dt_inception_features launch sequence)."""
        x = self._images(images)
        N, C, H, W = x.shape
        if out is None:
            out = torch.empty(N, N_FEATURES, dtype=torch.float32, device=self.device)
        ws = self.workspace(N)
        with torch.cuda.device(self.device):
            check(_hip.load().dt_inception_features(self._h, ptr(x), N, C, H, W, in_scale, in_shift, ptr(out), ptr(ws),
                                                    ws.numel(), stream_ptr()), "dt_inception_features")
        return out

    def run_modules(self, x, first, last):
        """Modules [first, last) on x, the NHWC input of module ``first``; returns the NHWC output of module last - 1
        ([N, 2048] for the avgpool module)."""
        if not (0 <= first < last <= len(MODULES)):
            raise ValueError(f"module range [{first}, {last}) outside [0, {len(MODULES)})")
        (H, W, C), _ = module_shape(first)
        _, (OH, OW, OC) = module_shape(last - 1)
        if x.dim() != 4 or tuple(x.shape[1:]) != (H, W, C):
            raise ValueError(f"{MODULES[first]} takes [N, {H}, {W}, {C}], got {tuple(x.shape)}")
        x = x.detach().to(self.device, torch.float32).contiguous()
        N = x.shape[0]
        shape = (N, OC) if last == len(MODULES) else (N, OH, OW, OC)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        ws = self.workspace(N)
        with torch.cuda.device(self.device):
            check(_hip.load().dt_inception_run_modules(self._h, first, last, ptr(x), N, ptr(out), ptr(ws), ws.numel(),
                                                       stream_ptr()), "dt_inception_run_modules")
        return out
