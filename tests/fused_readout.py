"""Reading one U-Net block at a time out of a forward that stores no activation (csrc/dt_fused.hip keeps every one in LDS).

The layer table of the fused kernel depends on the channel counts alone, never on the weights.  So block j is observed
through weights: a block whose norm2 weight and bias are zero outputs exactly its skip path (``transparent``), a 0 / 1
``residual_conv`` with zero bias is an exact selection, and a 0 / 1 ``final`` selects the C channels that reach eps.  In
M(j, k) the blocks 0 .. j keep their weights, the blocks j + 1 .. 7 are transparent, and eps is a fixed linear readout of
block j's output: select C channels, (enc1 only) the 2x2 max pool, x2 bilinear upsamples back to 16 x 16 --

  j   block       carried by                                   readout of block j's output
  -1  (image)     enc1, enc2 selections, then route 1 .. 4     pool^r, up^r    (r = route: x2, x3, x4, bottleneck)
  0   enc1        pool, enc2's selection, dec1's skip half     pool, up
  1   enc2        dec1's skip half                             up
  2   enc3        dec2's skip half, dec1's upsampled half      up^2
  3   enc4        dec3's skip half, dec2 / dec1 upsampled      up^3
  4   bottleneck  dec3 / dec2 / dec1 upsampled halves          up^4
  5   dec3        dec2 / dec1 upsampled halves                 up^3
  6   dec2        dec1's upsampled half                        up^2
  7   dec1        the head                                     up

(enc1's unpooled output is used by nothing in this network: its pooled values are the whole observable.)  Over k the
selected channel groups cover every real output channel of block j.  The positions the carried channels take in the
blocks downstream move with k and with the block (``_place``), so the channels next to the padding boundary and both
halves of every decoder concat are read.  tests/test_fused_readout_host.py proves the surgery exact in float64 without a
GPU; tests/test_hip_fused_blocks.py and tools/fuzz_fused.py use it on the device.
"""
from typing import NamedTuple

import torch
import torch.nn.functional as F

from oracle import unet_ref

BLOCKS = unet_ref.BLOCKS
MARGIN = 4            # the margin tests/test_hip_conv_blocks.py keeps over its measured maximum
POOLS_UPS = {0: (1, 1), 1: (0, 1), 2: (0, 2), 3: (0, 3), 4: (0, 4), 5: (0, 3), 6: (0, 2), 7: (0, 1)}


def transparent(sd32, j, sel=None):
    """the weights with block j made transparent: norm2's weight and bias zero, so relu(bn2(conv2)) is exactly 0 and the block
    output is its skip path alone -- the input itself (identity skips), or, where the block has a 1x1 residual_conv, a 0 / 1
    selection with zero bias: output channel n = input channel sel[n] (no weight at all where sel[n] < 0); without ``sel``,
    input channel n % cin"""
    sd, name = dict(sd32), BLOCKS[j]
    for key in (f"{name}.norm2.weight", f"{name}.norm2.bias"):
        sd[key] = torch.zeros_like(sd[key])
    if f"{name}.residual_conv.weight" in sd:
        w = torch.zeros_like(sd[f"{name}.residual_conv.weight"])
        cout, cin = w.shape[:2]
        sel = torch.arange(cout) % cin if sel is None else torch.as_tensor(sel)
        assert sel.shape == (cout,) and int(sel.max()) < cin
        on = sel >= 0
        w[torch.arange(cout)[on], sel[on], 0, 0] = 1.0
        sd[f"{name}.residual_conv.weight"] = w
        sd[f"{name}.residual_conv.bias"] = torch.zeros_like(sd[f"{name}.residual_conv.bias"])
    else:
        assert sel is None, f"{name} has an identity skip"
    return sd


class Readout(NamedTuple):
    j: int            # the block read (-1: the image)
    k: int
    sd: dict          # M(j, k), fp32
    chans: tuple      # eps channel i carries channel chans[i] of block j's output (of the image for j = -1)
    pools: int        # 2x2 max pools between block j's output and eps
    ups: int          # x2 bilinear upsamples between block j's output and eps


def _up(a):
    return F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=True)


def readout(act, r):
    """the fixed linear map (a maximum aside) from block r.j's output [rows, c, h, w] to the eps of M(j, k)"""
    v = act
    for _ in range(r.pools):
        v = F.max_pool2d(v, 2)
    for _ in range(r.ups):
        v = _up(v)
    return v[:, list(r.chans)]


def channel_groups(cout, C):
    """first channels of the groups of C consecutive channels that cover 0 .. cout - 1 (the last group overlaps its neighbour
    where C does not divide cout)"""
    starts = list(range(0, cout - C + 1, C))
    if starts[-1] + C < cout:
        starts.append(cout - C)
    return starts


def _place(shift, b, n, cout):
    """output channels of selecting block b that carry the n read channels: consecutive (mod cout), moved by the group and by
    the block, so that over k every channel quad of every downstream tensor -- the last real one included -- is a carrier"""
    return [(shift + 5 * b + i) % cout for i in range(n)]


def surgery(sd32, j, chans, route=None, fill="wrap"):
    """M(j, k) for the channels ``chans`` of block j: (state dict, channels of dec1's output that ``final`` selects).

    ``route`` (j <= 4) names the encoder tensor that carries the channels into the decoder: 1 .. 4 = enc2 / enc3 / enc4 /
    bottleneck output; a block's own output for j = 1 .. 4, enc2's for j = 0, any of the four for the image (j = -1).
    ``fill``: what the output channels of a selecting block that are not carriers select -- "wrap": input channel n % cin
    (every channel of every tensor stays live, so a read from a neighbouring channel shows), "none": no weight (they are 0)."""
    assert fill in ("wrap", "none")
    if route is None:
        route = max(j, 1)
    assert (j <= 0 and 1 <= route <= 4 and (j < 0 or route == 1)) or route == j or j >= 5
    sd, cur, shift = dict(sd32), list(chans), chans[0]

    def select(b, offset, carry=True):
        nonlocal sd, cur
        cout, cin = sd32[f"{BLOCKS[b]}.residual_conv.weight"].shape[:2]
        sel = torch.arange(cout) % cin if fill == "wrap" else torch.full((cout,), -1)
        if carry:
            pos = _place(shift, b, len(cur), cout)
            sel[pos] = torch.tensor(cur) + offset
            cur = pos
        sd = transparent(sd, b, sel)

    if j < 0:
        select(0, 0)
    if j < 1:
        select(1, 0)
    for b in (2, 3, 4):
        if b > j:
            sd = transparent(sd, b)                       # identity skips: the output is the pooled input
    in_decoder = j >= 5
    for b, skip_level in ((5, 3), (6, 2), (7, 1)):
        if b <= j:
            continue
        half = sd32[f"{BLOCKS[b]}.residual_conv.weight"].shape[1] // 2      # cat([up(previous), encoder skip])
        if in_decoder or (route == 4 and b == 5):
            select(b, 0)
            in_decoder = True
        elif route == skip_level:
            select(b, half)
            in_decoder = True
        else:
            select(b, 0, carry=False)
    assert in_decoder
    w = torch.zeros_like(sd32["final.weight"])
    w[torch.arange(len(cur)), torch.tensor(cur), 0, 0] = 1.0
    sd["final.weight"], sd["final.bias"] = w, torch.zeros_like(sd32["final.bias"])
    return sd, tuple(cur)


def block_width(sd32, j):
    """real output channels of block j (image channels for j = -1)"""
    return sd32["final.weight"].shape[0] if j < 0 else sd32[f"{BLOCKS[j]}.conv2.weight"].shape[0]


def readout_models(sd32, j, fill="wrap"):
    """the Readouts M(j, k), k = 0, 1, ..: together they read every real output channel of block j.  j = -1 (every block
    transparent): the four routes of the image, its C channels rotated by the route"""
    C = sd32["final.weight"].shape[0]
    if j < 0:
        for k, route in enumerate((1, 2, 3, 4)):
            chans = tuple((i + k) % C for i in range(C))
            yield Readout(j, k, surgery(sd32, j, chans, route, fill)[0], chans, route, route)
        return
    for k, start in enumerate(channel_groups(block_width(sd32, j), C)):
        chans = tuple(range(start, start + C))
        yield Readout(j, k, surgery(sd32, j, chans, None, fill)[0], chans, *POOLS_UPS[j])


# ------------------------------------------------------------------ the block chain, in any precision
def forward_blocks(sd, x, temb, acts=None, start=0, block=unet_ref.block_forward):
    """(eps, [outputs of the eight blocks]) of oracle/unet_ref.unet_forward's block chain in the dtype of ``sd`` / ``x`` /
    ``temb`` [rows, D]; blocks below ``start`` are not evaluated, their outputs are taken from ``acts`` (the blocks 0 .. j
    of every M(j, k) carry the same weights).  ``block(sd, name, x, temb)`` evaluates one block."""
    a = list(acts[:start]) if start else []
    for j in range(start, 8):
        if j == 0:
            xin = x
        elif j <= 4:
            xin = F.max_pool2d(a[j - 1], 2)
        else:
            xin = torch.cat([_up(a[j - 1]), a[8 - j]], dim=1)
        a.append(block(sd, BLOCKS[j], xin, temb))
    return F.conv2d(_up(a[7]), sd["final.weight"], sd["final.bias"]), a


def forward64(sd64, x64, temb64, acts=None, start=0):
    """float64 reference: the block chain through unet_ref.block_forward on widened weights, with the time embedding taken
    in fp32 (``row_temb``) and widened -- the device's time_bias_kernel has its own test"""
    assert x64.dtype == torch.float64 and temb64.dtype == torch.float64
    with torch.no_grad():
        return forward_blocks(sd64, x64, temb64, acts, start)


def widen(sd32):
    return {k: v.double() for k, v in sd32.items() if v.dtype.is_floating_point}


# ------------------------------------------------------------------ batch rows
COND_NONE, COND_ZERO, COND_ONE = 0, 1, 2      # distillation_trajectories_amd._hip


class Layout(NamedTuple):
    """rows of one device call: [pass 0 of all B images | passes 1 .. of the images single ..]; row r takes the time-bias row
    r // tb_div, whose (t, cond mode) is conds[r // tb_div]"""
    name: str
    B: int
    n_pass: int
    single: int       # > 0: dt_unet_forward_mixed
    tb_div: int
    conds: tuple


def row_images(lay):
    return list(range(lay.B)) + [b for _ in range(lay.n_pass - 1) for b in range(lay.single, lay.B)]


def row_temb(sd32, lay):
    """fp32 [rows, D] time embedding of every batch row (oracle/unet_ref.time_embedding)"""
    t = torch.tensor([tc[0] for tc in lay.conds], dtype=torch.long)
    n = len(lay.conds)
    with torch.no_grad():
        embs = {COND_NONE: unet_ref.time_embedding(sd32, t, None),
                COND_ZERO: unet_ref.time_embedding(sd32, t, torch.zeros(n, 1)),
                COND_ONE: unet_ref.time_embedding(sd32, t, torch.ones(n, 1))}
    temb = torch.stack([embs[m][i] for i, (_, m) in enumerate(lay.conds)])
    return temb.repeat_interleave(lay.tb_div, dim=0)


class Inputs(NamedTuple):
    x: torch.Tensor          # [B, C, 16, 16] fp32: what the device call takes
    x_rows: torch.Tensor     # [rows, C, 16, 16]: the image of every batch row
    temb: torch.Tensor       # [rows, D] fp32 time embedding of every batch row
    acts32: list             # block outputs of the unchanged model, fp32 CPU oracle ...
    acts64: list             # ... and float64: blocks 0 .. j of every M(j, k) carry these weights


def make_inputs(sd32, lay, x):
    x_rows = x[row_images(lay)]
    temb = row_temb(sd32, lay)
    with torch.no_grad():
        acts32 = forward_blocks(sd32, x_rows, temb)[1]
    acts64 = forward64(widen(sd32), x_rows.double(), temb.double())[1]
    return Inputs(x, x_rows, temb, acts32, acts64)


def references(inp, r):
    """(float64 reference, fp32 CPU oracle) eps [rows, C, 16, 16] of the readout model r: the blocks downstream of r.j are
    evaluated, the outputs of blocks 0 .. r.j are the unchanged model's (tests/test_fused_readout_host.py checks both
    shortcuts against the evaluation from the image)"""
    start = max(r.j + 1, 0)
    ref64 = forward64(widen(r.sd), inp.x_rows.double(), inp.temb.double(), inp.acts64, start)[0]
    with torch.no_grad():
        cpu32 = forward_blocks(r.sd, inp.x_rows, inp.temb, inp.acts32, start)[0]
    return ref64, cpu32


# ------------------------------------------------------------------ the criterion
def row_errors(got, ref64):
    """(worst row's relative L2 error over the row's concatenated readouts, worst row's max-abs error over the row's max-abs
    reference) of got [K, rows, C, H, W] against ref64 of the same shape"""
    d = (got.double() - ref64).transpose(0, 1).flatten(1)
    r = ref64.transpose(0, 1).flatten(1)
    l2 = d.norm(dim=1) / r.norm(dim=1)
    ma = d.abs().amax(dim=1) / r.abs().amax(dim=1)
    return float(torch.nan_to_num(l2, nan=float("inf")).max()), float(torch.nan_to_num(ma, nan=float("inf")).max())


def within_margin(err, yardsticks):
    """each of the two quantities at most MARGIN times the larger of the yardsticks' (a NaN or Inf error fails)"""
    return all(err[i] <= MARGIN * max(y[i] for y in yardsticks) for i in range(2))


# ------------------------------------------------------------------ on the device
def device_eps(h, x_dev, lay):
    """eps [rows, C, 16, 16] of one device call in the layout's row order, on whichever path the handle is set to"""
    tb = h.time_bias([t for t, _ in lay.conds], [m for _, m in lay.conds])
    if lay.single:
        return h.forward_mixed(x_dev, tb, lay.single, lay.tb_div)
    return h.forward(x_dev, tb, lay.n_pass, lay.tb_div)


class Measured(NamedTuple):
    fused: tuple        # row_errors of the fused kernel against float64 ...
    layered: tuple      # ... of the layered kernels (set_fused(False), PREC_FP32) ...
    cpu: tuple          # ... and of the fp32 CPU oracle: the two yardsticks
    cross: tuple        # row_errors of the fused eps against the layered eps
    eps: dict           # "fused" / "layered" / "cpu" / "ref64" -> [K, rows, C, 16, 16] on the host
    models: list        # the Readouts

    def ok(self):
        """the criterion: the fused kernel's error against float64, and its distance from the layered path, within MARGIN of
        the larger yardstick"""
        return within_margin(self.fused, [self.layered, self.cpu]) and within_margin(self.cross, [self.layered, self.cpu])

    def line(self):
        f = lambda e: f"{e[0]:.2e} {e[1]:.2e}"
        return f"fused {f(self.fused)} | layered {f(self.layered)} | cpu fp32 {f(self.cpu)} | fused-layered {f(self.cross)}"


def measure_block(sd32, j, layouts, inputs, device, fill="wrap", only=None):
    """{layout name: Measured} of block j: one handle per M(j, k) (``only``: these k), every layout on the fused kernel and on
    the layered fp32 kernels, against forward64 and the fp32 CPU oracle of the same M(j, k) on the same inputs"""
    from distillation_trajectories_amd import _hip, engine
    got = {lay.name: dict(fused=[], layered=[], cpu=[], ref64=[]) for lay in layouts}
    models = [r for r in readout_models(sd32, j, fill) if only is None or r.k in only]
    for r in models:
        h = engine.UNetHandle(r.sd, device)
        assert h.fused_active(16, 16), "the model does not take the fused kernel"
        for lay in layouts:
            got[lay.name]["fused"].append(device_eps(h, inputs[lay.name].x.to(device), lay).cpu())
        h.set_fused(False)
        h.set_precision(_hip.PREC_FP32)
        assert not h.fused_active(16, 16)
        for lay in layouts:
            got[lay.name]["layered"].append(device_eps(h, inputs[lay.name].x.to(device), lay).cpu())
            ref64, cpu32 = references(inputs[lay.name], r)
            got[lay.name]["ref64"].append(ref64), got[lay.name]["cpu"].append(cpu32)
    out = {}
    for lay in layouts:
        e = {k: torch.stack(v) for k, v in got[lay.name].items()}
        out[lay.name] = Measured(row_errors(e["fused"], e["ref64"]), row_errors(e["layered"], e["ref64"]), row_errors(e["cpu"], e["ref64"]),
                                 row_errors(e["fused"], e["layered"].double()), e, models)
    return out
