"""LPIPS v0.1 with ``net='alex'`` on libdt_hip (include/dt_hip_lpips.h): the perceptual distance of the reference's
``evaluation/metrics.py compute_lpips``.

The network is torchvision AlexNet's ``features`` up to the fifth ReLU behind the LPIPS scaling layer; the distance is the
pixel mean of the channel-normalised squared feature differences weighted by the five 1x1 "lin" layers, summed over the
five ReLU maps.  Weights are the user's own: given as a path or a mapping, or named by ``DT_LPIPS_WEIGHTS``; nothing is
ever downloaded and there is no placeholder value.

Two weight layouts are accepted (``KEYS`` below is the one table of their key names).  The names are written down from
memory of the ``lpips`` and ``torchvision`` packages; neither is installed where this was written, so they could not be
checked against the packages themselves.  If a release names a tensor differently, ``KEYS`` is the only place to change.

  (a) one state dict of ``lpips.LPIPS(net='alex')``: convs under ``net.slice{1..5}.{0,3,6,8,10}``, lins under
      ``lin{k}.model.1.weight`` (``lins.{k}.model.1.weight`` is the same tensor under its ModuleList name; both are accepted),
      ``scaling_layer.*`` accepted and ignored;
  (b) a pair: torchvision's AlexNet state dict (``features.{0,3,6,8,10}.*``; ``classifier.*`` ignored) and the ``lpips``
      package's ``alex.pth`` (``lin{k}.model.1.weight``).
"""
import os
from collections.abc import Mapping
from ctypes import c_int

import torch

from . import _hip
from ._hip import check, ptr, stream_ptr

WEIGHTS_ENV = "DT_LPIPS_WEIGHTS"
N_LAYERS = 5
MIN_SIZE, MAX_SIZE = 31, 299
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (cin, cout, kernel, stride, padding, a 3x3 s2 max pool in front) of the five convs, each followed by bias + ReLU
CONVS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False),
         (256, 256, 3, 1, 1, False))
CHANNELS = tuple(c[1] for c in CONVS)
_FEATURE_INDEX = (0, 3, 6, 8, 10)          # the convs' positions in torchvision's AlexNet.features

# the key table: per layout, the prefix of conv k (0-based) and the accepted names of lin k, first the canonical one
KEYS = {
    "lpips": {"conv": tuple(f"net.slice{k + 1}.{i}" for k, i in enumerate(_FEATURE_INDEX)),
              "lin": tuple((f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight") for k in range(N_LAYERS)),
              "ignored": ("scaling_layer.",)},
    "torchvision": {"conv": tuple(f"features.{i}" for i in _FEATURE_INDEX), "ignored": ("classifier.",)},
    "lins": {"lin": tuple((f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight") for k in range(N_LAYERS)),
             "ignored": ()},
}


def conv_shape(k):
    cin, cout, ks = CONVS[k][:3]
    return (cout, cin, ks, ks)


def key_table(layout="lpips"):
    """{key: shape} of every tensor a layout may hold that the network uses (aliases included)."""
    rows = {}
    for k, prefix in enumerate(KEYS[layout].get("conv", ())):
        rows[f"{prefix}.weight"] = conv_shape(k)
        rows[f"{prefix}.bias"] = (CONVS[k][1],)
    for k, names in enumerate(KEYS[layout].get("lin", ())):
        for name in names:
            rows[name] = (1, CHANNELS[k], 1, 1)
    return rows


def _take(state_dict, layout, what):
    """The conv tensors and / or lin tensors of one mapping, checked against the layout's table."""
    if not isinstance(state_dict, Mapping):
        raise ValueError(f"LPIPS weights ({layout} layout): expected a state dict, got {type(state_dict).__name__}")
    table = key_table(layout)
    for key, v in state_dict.items():
        if key not in table:
            if key.startswith(KEYS[layout]["ignored"]) and KEYS[layout]["ignored"]:
                continue
            raise ValueError(f"LPIPS weights ({layout} layout): unexpected key '{key}'")
        if tuple(v.shape) != table[key]:
            raise ValueError(f"LPIPS weights ({layout} layout): '{key}' has shape {tuple(v.shape)}, expected {table[key]}")
    convs, lins = [], []
    if "conv" in what:
        for prefix in KEYS[layout]["conv"]:
            for leaf in ("weight", "bias"):
                if f"{prefix}.{leaf}" not in state_dict:
                    raise ValueError(f"LPIPS weights ({layout} layout): missing key '{prefix}.{leaf}'")
                convs.append(state_dict[f"{prefix}.{leaf}"])
    if "lin" in what:
        for names in KEYS[layout]["lin"]:
            found = [n for n in names if n in state_dict]
            if not found:
                raise ValueError(f"LPIPS weights ({layout} layout): missing key '{names[0]}'")
            lins.append(state_dict[found[0]])
    return convs, lins


def check_state_dict(weights):
    """The 15 tensors of dt_lpips_create, in its order (conv_k.weight, conv_k.bias for k = 1..5, then lin_0..lin_4), from
    layout (a), one mapping, or layout (b), a pair (torchvision AlexNet state dict, alex.pth).  A missing, mis-shaped or
    unknown key raises ValueError naming it."""
    if isinstance(weights, (tuple, list)):
        if len(weights) != 2:
            raise ValueError(f"LPIPS weights: a pair (AlexNet state dict, lin state dict) has 2 members, got {len(weights)}")
        convs, _ = _take(weights[0], "torchvision", ("conv",))
        _, lins = _take(weights[1], "lins", ("lin",))
    else:
        convs, lins = _take(weights, "lpips", ("conv", "lin"))
    return convs + lins


def _load(path):
    if not os.path.exists(path):
        raise FileNotFoundError(f"LPIPS weights file {path} does not exist")
    return torch.load(path, map_location="cpu", weights_only=True)


def read_weights(weights=None):
    """One mapping (layout (a)) or a pair of mappings (layout (b)) from ``weights``: a mapping, a path, a pair of either,
    or ``"alexnet.pth,alex.pth"``; default: what ``$DT_LPIPS_WEIGHTS`` names."""
    if weights is None:
        weights = os.environ.get(WEIGHTS_ENV) or None
    if weights is None:
        raise FileNotFoundError(
            f"no LPIPS weights: pass weights=<path or state dict> or set {WEIGHTS_ENV} to a state dict of "
            f"lpips.LPIPS(net='alex'), or to 'alexnet.pth,alex.pth' (torchvision's AlexNet state dict and the lpips "
            f"package's v0.1 lin weights). Weights are never downloaded and there is no placeholder distance.")
    if isinstance(weights, (str, os.PathLike)):
        parts = [p.strip() for p in os.fspath(weights).split(",")]
        if len(parts) > 2:
            raise ValueError(f"LPIPS weights: expected one path or 'alexnet.pth,alex.pth', got {weights!r}")
        weights = _load(parts[0]) if len(parts) == 1 else tuple(parts)
    if isinstance(weights, (tuple, list)):
        return tuple(_load(os.fspath(w)) if isinstance(w, (str, os.PathLike)) else w for w in weights)
    return weights


def check_size(H, W):
    if not (MIN_SIZE <= H <= MAX_SIZE and MIN_SIZE <= W <= MAX_SIZE):
        raise ValueError(f"LPIPS: image size {H}x{W} is outside {MIN_SIZE}..{MAX_SIZE} (below {MIN_SIZE} AlexNet's second "
                         f"max pool has nothing to pool; resize first)")


def check_images(images):
    """Raise ValueError unless ``images`` is an [N, 3, H, W] tensor with N >= 1 and 31 <= H, W <= 299."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError(f"LPIPS: images must be an [N, 3, H, W] tensor, got "
                         f"{tuple(images.shape) if isinstance(images, torch.Tensor) else type(images).__name__}")
    N, C, H, W = images.shape
    if C != 3:
        raise ValueError(f"LPIPS: images must have 3 channels, got {C}")
    check_size(H, W)
    if N < 1:
        raise ValueError("LPIPS: no images")


def layer_shapes(H, W):
    """[(H_l, W_l, C_l)] of the five ReLU maps for an H x W image: the table of include/dt_hip_lpips.h, in Python."""
    check_size(H, W)
    out, h, w = [], H, W
    for cin, cout, k, s, p, pool in CONVS:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        out.append((h, w, cout))
    return out


def layer_shape(H, W, l):
    """(H_l, W_l, C_l) of ReLU map l as the library's table has it."""
    d = (c_int * 3)()
    check(_hip.load().dt_lpips_layer_shape(H, W, l, d), "dt_lpips_layer_shape")
    return tuple(d)


def feature_floats(H, W):
    """Floats of one image's feature pack (the five ReLU maps, NHWC, one after another)."""
    check_size(H, W)
    return int(_hip.load().dt_lpips_feature_floats(H, W))


def split_pack(pack, H, W):
    """The five [N, H_l, W_l, C_l] views of a feature pack [N, floats]."""
    out, off = [], 0
    for h, w, c in layer_shapes(H, W):
        out.append(pack[:, off:off + h * w * c].view(-1, h, w, c))
        off += h * w * c
    return out


class LPIPSHandle(_hip.DeviceHandle):
    """The network's weights on one device (dt_lpips_create) and a workspace grown on demand: ``workspace(N, H, W)``."""
    ENTRY, GPU_ONLY = "dt_lpips", "LPIPS runs"

    def __init__(self, weights, device):
        super().__init__(check_state_dict(weights), device)

    def features(self, images, in_scale=1.0, in_shift=0.0, out=None):
        """[N, feature_floats(H, W)] fp32 on the device for images [N, 3, H, W]: ``in_scale * x + in_shift``, the
        scaling layer and the five layers (one dt_lpips_features launch sequence)."""
        check_images(images)
        x = images.detach().to(self.device, torch.float32).contiguous()
        N, C, H, W = x.shape
        if out is None:
            out = torch.empty(N, feature_floats(H, W), dtype=torch.float32, device=self.device)
        ws = self.workspace(N, H, W)
        with torch.cuda.device(self.device):
            check(_hip.load().dt_lpips_features(self._h, ptr(x), N, C, H, W, in_scale, in_shift, ptr(out), ptr(ws),
                                                ws.numel(), stream_ptr()), "dt_lpips_features")
        return out

    def run_layers(self, x, first, last, H, W):
        """Layers [first, last) for H x W images on x, the NHWC input of layer ``first`` (the scaled image
        [N, H, W, 3] for layer 0, ReLU map first - 1 otherwise); returns ReLU map last - 1, NHWC."""
        if not (0 <= first < last <= N_LAYERS):
            raise ValueError(f"layer range [{first}, {last}) outside [0, {N_LAYERS})")
        shapes = layer_shapes(H, W)
        want = (H, W, 3) if first == 0 else shapes[first - 1]
        if x.dim() != 4 or tuple(x.shape[1:]) != want:
            raise ValueError(f"layer {first} takes [N, {want[0]}, {want[1]}, {want[2]}], got {tuple(x.shape)}")
        x = x.detach().to(self.device, torch.float32).contiguous()
        N = x.shape[0]
        out = torch.empty((N,) + shapes[last - 1], dtype=torch.float32, device=self.device)
        ws = self.workspace(N, H, W)
        with torch.cuda.device(self.device):
            check(_hip.load().dt_lpips_run_layers(self._h, first, last, ptr(x), N, H, W, ptr(out), ptr(ws), ws.numel(),
                                                  stream_ptr()), "dt_lpips_run_layers")
        return out

    def _pack(self, t, name, F, dims):
        if not isinstance(t, torch.Tensor) or t.dim() != dims or t.shape[-1] != F or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 feature pack with {dims} dimensions and {F} floats per image, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        return t.to(self.device).contiguous()

    def distance(self, pack0, pack1, H, W, per_layer=False):
        """[n1] distances between pack0 [n0, F] (n0 = 1: one image shared by all) and pack1 [n1, F]; with ``per_layer``
        also the five terms, [n1, 5]."""
        F = feature_floats(H, W)
        p0, p1 = self._pack(pack0, "pack0", F, 2), self._pack(pack1, "pack1", F, 2)
        n0, n1 = p0.shape[0], p1.shape[0]
        if n1 < 1 or n0 not in (1, n1):
            raise ValueError(f"pack0 holds {n0} images and pack1 {n1}: pack0 must hold one image or as many as pack1")
        dist = torch.empty(n1, dtype=torch.float32, device=self.device)
        layers = torch.empty(n1, N_LAYERS, dtype=torch.float32, device=self.device) if per_layer else None
        with torch.cuda.device(self.device):
            check(_hip.load().dt_lpips_distance(self._h, ptr(p0), n0, ptr(p1), n1, H, W, ptr(dist), ptr(layers),
                                                stream_ptr()), "dt_lpips_distance")
        return (dist, layers) if per_layer else dist

    def distance_many(self, pack0, pack1, H, W, per_layer=False):
        """[G, n] distances of pack0 [n, F] against each of pack1 [G, n, F] in one launch (pair (g, i): pack0[i] and
        pack1[g][i]); with ``per_layer`` also [G, n, 5]."""
        F = feature_floats(H, W)
        p0, p1 = self._pack(pack0, "pack0", F, 2), self._pack(pack1, "pack1", F, 3)
        n, G = p0.shape[0], p1.shape[0]
        if n < 1 or G < 1 or p1.shape[1] != n:
            raise ValueError(f"pack1 {tuple(p1.shape)} does not hold G sets of pack0's {n} images")
        dist = torch.empty(G, n, dtype=torch.float32, device=self.device)
        layers = torch.empty(G, n, N_LAYERS, dtype=torch.float32, device=self.device) if per_layer else None
        with torch.cuda.device(self.device):
            check(_hip.load().dt_lpips_distance_many(self._h, ptr(p0), ptr(p1), n, G, H, W, ptr(dist), ptr(layers),
                                                     stream_ptr()), "dt_lpips_distance_many")
        return (dist, layers) if per_layer else dist
