"""LPIPS v0.1, net='alex', restated on torch-CPU ops: the yardstick of tests/test_lpips_host.py and
tests/test_hip_lpips.py.  It runs in the dtype of the state dict it is given: float64 is the reference, float32 (the
arithmetic the ``lpips`` package itself runs) is the yardstick whose own error against float64 sets the distance bounds.

The state dict uses layout (a) of distillation_trajectories_amd/lpips.py, the key names of ``lpips.LPIPS(net='alex')``.
"""
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (state-dict prefix, cin, cout, kernel, stride, padding, max pool 3x3 s2 in front)
LAYERS = (("net.slice1.0", 3, 64, 11, 4, 2, False), ("net.slice2.3", 64, 192, 5, 1, 2, True),
          ("net.slice3.6", 192, 384, 3, 1, 1, True), ("net.slice4.8", 384, 256, 3, 1, 1, False),
          ("net.slice5.10", 256, 256, 3, 1, 1, False))
SIZES = ((31, 31), (32, 32), (35, 47), (64, 64))
PAIRS_PER_SIZE = 8


def random_state_dict(seed, dtype=torch.float64):
    """conv weights N(0, 2 / fan_in), biases 0.1 N(0, 1), lin weights U(0, 1); scaling_layer buffers included."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cin, cout, k, *_ in LAYERS:
        sd[f"{name}.weight"] = (torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) * (2.0 / (cin * k * k)) ** 0.5)
        sd[f"{name}.bias"] = 0.1 * torch.randn(cout, generator=g, dtype=torch.float64)
    for l, (_, _, cout, *_) in enumerate(LAYERS):
        sd[f"lin{l}.model.1.weight"] = torch.rand(1, cout, 1, 1, generator=g, dtype=torch.float64)
    sd["scaling_layer.shift"] = torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    return cast(sd, dtype)


def cast(sd, dtype):
    """The fp32 state dict is the float64 one rounded, so both describe the same network up to that rounding; the
    float64 reference of an fp32 run uses ``cast(cast(sd, float32), float64)``."""
    return {k: v.to(dtype) for k, v in sd.items()}


def images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tanh(1.5 * torch.randn(n, 3, h, w, generator=g))


def _dtype(sd):
    return sd["net.slice1.0.weight"].dtype


def scale_input(sd, x, in_scale=1.0, in_shift=0.0):
    """[N, 3, H, W] -> the scaling layer's output, in the state dict's dtype."""
    dt = _dtype(sd)
    v = in_scale * x.to(dt) + in_shift
    shift, scale = (torch.tensor(c, dtype=dt, device=v.device).view(1, 3, 1, 1) for c in (SHIFT, SCALE))
    return (v - shift) / scale


def run_layer(sd, l, x):
    """Layer l (its pool, conv, bias, ReLU) on x NCHW: the scaled image for l = 0, ReLU map l - 1 otherwise."""
    name, _, _, _, stride, pad, pool = LAYERS[l]
    x = x.to(_dtype(sd))
    if pool:
        x = F.max_pool2d(x, kernel_size=3, stride=2)
    return F.relu(F.conv2d(x, sd[f"{name}.weight"], sd[f"{name}.bias"], stride=stride, padding=pad))


def taps(sd, x, in_scale=1.0, in_shift=0.0):
    """The five ReLU maps, NCHW."""
    out, y = [], scale_input(sd, x, in_scale, in_shift)
    for l in range(len(LAYERS)):
        y = run_layer(sd, l, y)
        out.append(y)
    return out


def distance_from_taps(sd, t0, t1):
    """[N, 5] layer terms; the distance is their sum."""
    terms = []
    for l, (a, b) in enumerate(zip(t0, t1)):
        na = a / (a.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        nb = b / (b.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        w = sd[f"lin{l}.model.1.weight"]
        terms.append((w * (na - nb) ** 2).sum(dim=1).mean(dim=(1, 2)))
    return torch.stack(terms, dim=1)


def distance(sd, x0, x1, in_scale=1.0, in_shift=0.0):
    """([N] distances, [N, 5] layer terms) between images x0 and x1 ([N, 3, H, W]; x0 may hold one image)."""
    if x0.shape[0] == 1 and x1.shape[0] > 1:
        x0 = x0.expand(x1.shape[0], -1, -1, -1)
    terms = distance_from_taps(sd, taps(sd, x0, in_scale, in_shift), taps(sd, x1, in_scale, in_shift))
    return terms.sum(dim=1), terms


def pair_inputs(hw, kind, n=PAIRS_PER_SIZE):
    """The committed inputs of the distance checks, images in [-1, 1] (map (1, 0)): ``independent`` images, or ``near``
    pairs a, a + 0.05 randn, whose feature differences cancel."""
    h, w = hw
    a = images(n, h, w, seed=1000 + 10 * h + w)
    if kind == "independent":
        return a, images(n, h, w, seed=5000 + 10 * h + w)
    assert kind == "near"
    g = torch.Generator().manual_seed(9000 + 10 * h + w)
    return a, a + 0.05 * torch.randn(a.shape, generator=g)


def relative_errors(got, got_layers, want, want_layers):
    """(max relative error of the totals, max relative error of the layer terms) against float64 values."""
    total = ((got.double() - want).abs() / want.abs()).max().item()
    per = ((got_layers.double() - want_layers).abs() / want_layers.abs()).max().item()
    return total, per


def yardstick(sd32, kind):
    """Max relative error (total, per layer) of the fp32 restatement against the float64 one over SIZES, for one kind of
    pair.  Both run the SAME fp32 weights."""
    sd64 = cast(sd32, torch.float64)
    worst_t = worst_l = 0.0
    for hw in SIZES:
        a, b = pair_inputs(hw, kind)
        d32, l32 = distance(sd32, a, b)
        d64, l64 = distance(sd64, a, b)
        t, p = relative_errors(d32, l32, d64, l64)
        worst_t, worst_l = max(worst_t, t), max(worst_l, p)
    return worst_t, worst_l
