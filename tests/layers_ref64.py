"""float64 restatements of the layer kernels around the convolutions (csrc/dt_layers.hip), each with its magnitude bound.

  time_tower / time_tower_bound   sinusoidal embedding, time / condition MLPs, per-block time projection
                                  (reference models.py:15-39, 175-185, 66-77; time_bias_kernel)
  class_biases                    the nine class-bias vectors of enc1.conv2 (tap_bias_kernel)
  head                            conv1x1(bilinear_x2(dec1, align_corners=True)) + bias (head_kernel + head_upsample_kernel,
                                  eps_from_lowres of the sampler's update)

A bound S is the same evaluation with every weight, bias and intermediate replaced by its magnitude (block_bound of
tests/test_hip_conv_blocks.py): an fp32 evaluation in any summation order differs from float64 by a small multiple of
2^-24 * S, whatever cancels inside the sums.  CPU only (torch); tests/test_layers_ref64.py checks these functions against the
fp32 oracle, tests/test_hip_layers.py holds the kernels to them.
"""
import torch
import torch.nn.functional as F

BLOCKS = ("enc1", "enc2", "enc3", "enc4", "bottleneck", "dec3", "dec2", "dec1")


def _rows(t, cond, present):
    """(t float32 [rows], cond float64 [rows], has_cond bool [rows]); a null cond means no row has a condition, a null present
    (with a cond) that every row has one -- dt_unet_time_bias's convention"""
    t32 = torch.as_tensor(t).reshape(-1).to(torch.float32)          # the kernel converts the int32 t to fp32
    rows = t32.numel()
    if cond is None:
        return t32, torch.zeros(rows, dtype=torch.float64), torch.zeros(rows, dtype=torch.bool)
    c = torch.as_tensor(cond).reshape(-1).to(torch.float32).to(torch.float64)     # the condition is an fp32 input
    has = torch.ones(rows, dtype=torch.bool) if present is None else torch.as_tensor(present).reshape(-1) != 0
    return t32, c, has


def _embedding(D, freqs32, t32):
    """[rows, D] float64: sin / cos of the fp32 product t * freq (formed in fp32 by the reference and by the kernel alike),
    odd D with a trailing zero"""
    f32 = torch.as_tensor(freqs32).reshape(-1).to(torch.float32)
    arg = (t32[:, None] * f32[None, :]).double()                    # fp32 product, widened
    emb = torch.cat([arg.sin(), arg.cos()], dim=1)
    if emb.shape[1] < D:
        emb = torch.cat([emb, torch.zeros(emb.shape[0], D - emb.shape[1], dtype=torch.float64)], dim=1)
    return emb[:, :D]


def _tower(sd, emb, c, has, mag):
    """temb and per-block projections from the embedding; mag: every term by its magnitude (sd holds magnitudes then)"""
    temb = F.linear(emb, sd["time_mlp.1.weight"], sd["time_mlp.1.bias"])
    temb = temb if mag else torch.relu(temb)
    hid = F.linear(c[:, None], sd["cond_emb.0.weight"], sd["cond_emb.0.bias"])
    hid = hid if mag else torch.relu(hid)
    branch = F.linear(hid, sd["cond_emb.2.weight"], sd["cond_emb.2.bias"])
    temb = temb + branch * has[:, None].to(branch.dtype)            # no condition: the branch is absent, not evaluated at 0
    proj = {}
    for name in BLOCKS:
        p = F.linear(temb, sd[f"{name}.time_mlp.weight"], sd[f"{name}.time_mlp.bias"])
        proj[name] = p if mag else torch.relu(p)
    return temb, proj


_TOWER_KEYS = ("time_mlp.1.weight", "time_mlp.1.bias", "cond_emb.0.weight", "cond_emb.0.bias", "cond_emb.2.weight",
               "cond_emb.2.bias") + tuple(f"{n}.time_mlp.{k}" for n in BLOCKS for k in ("weight", "bias"))


def time_tower(sd64, freqs32, t, cond=None, present=None):
    """(temb [rows, D], {block: relu(time_mlp(temb)) [rows, cout]}) in float64.  freqs32: the handle's own fp32 frequency
    table (engine.sinusoid_frequencies); t integer [rows]; cond float [rows] or None; present 0 / 1 [rows] or None."""
    t32, c, has = _rows(t, cond, present)
    sd = {k: sd64[k].double() for k in _TOWER_KEYS}
    emb = _embedding(sd["time_mlp.1.weight"].shape[0], freqs32, t32)
    return _tower(sd, emb, c, has, False)


def time_tower_bound(sd64, freqs32, t, cond=None, present=None):
    """S of time_tower, same layout: every weight, bias and intermediate by its magnitude"""
    t32, c, has = _rows(t, cond, present)
    sd = {k: sd64[k].double().abs() for k in _TOWER_KEYS}
    emb = _embedding(sd["time_mlp.1.weight"].shape[0], freqs32, t32).abs()
    return _tower(sd, emb, c.abs(), has, True)


def tap_inside(cls, d):
    """whether tap offset d - 1 (d = 0, 1, 2) along an axis falls inside the picture for a pixel of class cls along that axis:
    0 first row / column (the tap before it is outside), 1 interior, 2 last (the tap after it is outside)"""
    return not (cls == 0 and d == 0) and not (cls == 2 and d == 2)


def class_biases(w2_64, b):
    """(vectors [..., 9, n], bound [..., 9, n]): for a spatially constant bias b [..., ci] in front of the zero-padded 3x3
    convolution w2 [n][ci][3][3], the sum over the taps INSIDE the picture of W2[n][ci][tap] b[ci]; class = 3 * cy + cx with
    cy, cx the class of the pixel's row / column (tap_inside)."""
    w, b = w2_64.double(), torch.as_tensor(b).double()
    out = []
    for per_tap in (torch.einsum("nckl,...c->...nkl", w, b), torch.einsum("nckl,...c->...nkl", w.abs(), b.abs())):
        vecs = []
        for cy in range(3):
            for cx in range(3):
                rows = [d for d in range(3) if tap_inside(cy, d)]
                cols = [d for d in range(3) if tap_inside(cx, d)]
                vecs.append(per_tap[..., rows, :][..., cols].sum(dim=(-2, -1)))
        out.append(torch.stack(vecs, dim=-2))
    return out[0], out[1]


def _up(a):
    return F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=True)


def axis_weights(n_in, dtype):
    """(i0, i1, l0, l1) of every output index of a bilinear x2 upsampling with align_corners=True along an axis of n_in
    pixels, the source coordinate and the two weights formed in ``dtype`` the way ATen forms them: scale = (in - 1) / (out - 1),
    src = scale * dst (a rounded product), l1 = src - floor(src), l0 = 1 - l1; returned as float64"""
    n_out = 2 * n_in
    scale = torch.tensor(n_in - 1, dtype=dtype) / torch.tensor(n_out - 1, dtype=dtype)
    src = scale * torch.arange(n_out).to(dtype)
    i0 = src.to(torch.int64)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = src - i0.to(dtype)
    l0 = 1 - l1
    return i0, i1, l0.double(), l1.double()


def _up_weights(a, dtype):
    """bilinear x2 of float64 a [..., h, w] with the weights of axis_weights(., dtype)"""
    y0, y1, wy0, wy1 = axis_weights(a.shape[-2], dtype)
    x0, x1, wx0, wx1 = axis_weights(a.shape[-1], dtype)
    top, bot = a[..., y0, :], a[..., y1, :]
    top = wx0 * top[..., x0] + wx1 * top[..., x1]
    bot = wx0 * bot[..., x0] + wx1 * bot[..., x1]
    return wy0[:, None] * top + wy1[:, None] * bot


def head(dec1_nchw64, final_w64, final_b64, coord32=False):
    """(eps [rows, C, 2h, 2w], bound): the reference's tail, conv1x1(bilinear_x2(dec1, align_corners=True)) + bias, and the
    same on |dec1|, |W|, |b| (the bilinear weights are non-negative).

    coord32: the interpolation weights are the fp32 numbers that ATen and the kernels form (axis_weights), everything else
    stays float64 -- the head without the rounding of the source coordinate, which is an error of up to 2^-23 * src in a
    weight and so grows with the picture's side."""
    d, w, b = dec1_nchw64.double(), final_w64.double(), final_b64.double()
    w = w.reshape(w.shape[0], -1, 1, 1)
    up = (lambda a: _up_weights(a, torch.float32)) if coord32 else _up
    return F.conv2d(up(d), w, b), F.conv2d(up(d.abs()), w.abs(), b.abs())
