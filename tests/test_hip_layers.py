"""The layer kernels around the convolutions (csrc/dt_layers.hip, csrc/dt_update.hip) at their edges.

a. Time tower (time_bias_kernel, tap_bias_kernel and the packs behind them) against float64 (tests/layers_ref64.py): every
   row of 1, 63, 64, 511, 512 and 515-row calls -- the 8-, 4- and 1-slice forms of launch_time_bias on both sides of both
   thresholds -- for D = 16, 25, 51, 76 and 256, conditions through dt_unet_time_bias's general form (a present table that
   mixes rows, condition values beyond 0 and 1, a null cond, a null present).  Projected columns are held to
   C_T * 2^-24 * S, class-bias columns to the same form (C_B) against the class biases of the device's own enc1 columns, padding
   columns are exactly 0, NaN- and 1e30-filled output buffers come out bit-identical and finite, and every row of every call
   is bit-identical to a one-row call of the same (t, cond, present): an output is one wave's dot product whose order
   depends on D alone.
b. Head (head_kernel, head_upsample_kernel) against float64 from the device's own dec1 output, head fusion off: channels
   1 .. 3, c_real 16, 25, 38, 64, 128, square and rectangular pictures, one and two passes, batches 1, 5, 41, and one case
   of 352256 low-resolution pixels, where head_kernel's grid of 8192 workgroups wraps.  (The fused head is tied to this one
   by tests/test_hip_conv_blocks.py.)
c. The interpolating update (cfg_update_kernel<RULE, LOWRES = true>, eps_from_lowres): one layered sampler step against
   forward + flat update (which test_cfg_update_bit_exact pins to torch CPU), bit for bit, on 16x48, 48x16 and 32x16
   pictures, every rule, one pass, two passes, per-row scales, mixed batches, row tables for the noise, masks and known
   images; the ENGINE dead step; a step of 528384 quads where the update's grid-stride loop (2048 workgroups) wraps; and a
   three-step loop against three chained one-step loops.

Measured on an MI355X against float64, maxima over all cases of a size factor (err / S in units of 2^-24).  Each constant
is the largest figure of its row times 4, rounded up to a power of two: other weights and shapes move a maximum by a small
factor, a dropped term or a shifted index by orders of magnitude.

  size factor                             0.05     0.1      0.2      0.3      0.5      1.0      large case
  time tower, projected columns  (C_T)    0.56     0.39     0.17     0.15     -        0.042
  time tower, class-bias columns (C_B)    1.74     1.53     1.50     1.49     -        1.72
  head, err / S                  (C_H)    11.52    -        9.20     5.93     5.61     4.54     10.76
  head, per-image relative L2    (REL_H)  6.63e-7  -        2.77e-7  5.10e-7  6.73e-7  6.74e-7  1.28e-7
  head, fp32 weights, err / S    (C_HW)   2.71     -        2.21     1.47     1.38     1.05     2.95

The head's err / S grows with the picture's side (at size factor 0.05: 2.7 on 16 x 16, 11.5 on 16 x 48, 10.8 on 64 x 64): the kernels form
the bilinear source coordinate scale * dst in fp32 as ATen does (bilinear_src), which moves an interpolation weight by up to
2^-23 * src, while float64 interpolates with exact weights.  The last row is the same comparison with float64 given the fp32
weights (layers_ref64.head(coord32=True)): what remains is the rounding of the sums, and it is held to its own constant.
"""
import random
from collections import defaultdict
from ctypes import c_size_t

import pytest
import torch

import layers_ref64 as ref64
from distillation_trajectories_amd import engine
from distillation_trajectories_amd._hip import (COND_NONE, COND_ONE, COND_ZERO, RULE_ENGINE, RULE_MANAGER, RULE_PSAMPLE, check, ptr,
                                                stream_ptr)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
C_T = 4                # time tower, projected columns: |got - ref64| <= C_T * 2^-24 * S (measured max 0.56)
C_B = 8                # time tower, class-bias columns against class_biases of the device's own enc1 columns (measured max 1.74)
C_H = 64               # head: |eps - ref64| <= C_H * 2^-24 * S (measured max 11.52)
REL_H = 2.0 ** -18     # head: per-image relative L2 error against float64 (measured max 6.74e-7)
C_HW = 16              # head against float64 with the fp32 interpolation weights (measured max 2.95)
POISONS = (float("nan"), 1e30)   # fmaxf-style ReLUs turn a NaN read into 0: a large finite value is needed too
RULES = (RULE_ENGINE, RULE_PSAMPLE, RULE_MANAGER)


@pytest.fixture(scope="module")
def cpu_threads():
    """float64 references on at most 16 threads (a GPU box may show many more cores than a job may use)"""
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(old, 16)))
    yield
    torch.set_num_threads(old)


@pytest.fixture(scope="module")
def stats():
    """per (kernel, size factor): the largest figure seen"""
    table = defaultdict(float)
    yield table
    print("\nmaxima against float64 (err / S in units of 2^-24; relative L2 per image):")
    for key in sorted(table):
        print(f"  {key[0]} sf {key[1]}: {table[key]:.3e}")


@pytest.fixture(scope="module")
def handles():
    """(handle, fp32 state dict) per (size factor, channels, purpose): 'head' runs the layered kernels with the head as
    launches of its own, 'layered' the layered kernels as the sampler runs them, 'tower' is the default handle"""
    cache = {}

    def get(sf, channels=3, purpose="tower"):
        key = (sf, channels, purpose)
        if key not in cache:
            from distillation_trajectories_amd.config import Config
            from distillation_trajectories_amd.models import DiffusionUNet
            from distillation_trajectories_amd.synthetic import make_model
            cfg = Config()
            cfg.image_size, cfg.channels = 16, channels
            sd32 = {k: v.float() for k, v in make_model(DiffusionUNet, cfg, sf).state_dict().items() if v.dtype.is_floating_point}
            h = engine.UNetHandle(sd32, DEV)
            if purpose != "tower":
                h.set_fused(False)
            if purpose == "head":
                h.set_head_fusion(False)
            cache[key] = (h, sd32)
        return cache[key]
    yield get
    cache.clear()


def bits(t):
    return t.contiguous().view(torch.int32)


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ a. time tower
ROW_COUNTS = (1, 63, 64, 511, 512, 515)     # launch_time_bias: 8 slices below 64 rows, 4 up to 511, 1 from 512 on
N_ROWS = max(ROW_COUNTS)
T_FIXED = (0, 1, 49, 999, 3920)
COND_VALUES = (0.0, 1.0, 0.37, -2.0, 2.5)
TOWER_SF = (0.05, 0.1, 0.2, 0.3, 1.0)       # D = 16 (fewer than 64 lanes), 25 (odd), 51 (25 / 50 channels in 32 / 64), 76, 256


def tower_rows():
    """(t, cond, present) of row r, the same in every call that has a row r"""
    rng = random.Random(2024)
    t = [T_FIXED[r % 6] if r % 6 < 5 else rng.randrange(0, 4000) for r in range(N_ROWS)]
    cond = [COND_VALUES[rng.randrange(5)] for _ in range(N_ROWS)]
    present = [rng.randrange(2) for _ in range(N_ROWS)]
    return t, cond, present


def tower_call(h, t, cond, present, rows, fill):
    """dt_unet_time_bias into a buffer filled beforehand"""
    out = torch.full((rows, h.tb_stride), fill, dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        check(h.lib.dt_unet_time_bias(h.h, ptr(t), ptr(cond), ptr(present), rows, ptr(out), stream_ptr()), "dt_unet_time_bias")
    return out


def tower_layout(sd32):
    """[(block, offset, cout, cout_p)], projected columns, c0, c0p"""
    lay, off = [], 0
    for name in ref64.BLOCKS:
        cout = sd32[f"{name}.time_mlp.weight"].shape[0]
        cp = (cout + 15) // 16 * 16
        lay.append((name, off, cout, cp))
        off += cp
    return lay, off, lay[0][2], lay[0][3]


def check_tower(got, sd32, sd64, freqs, t, cond, present, what, stats, sf):
    """one call's rows (CPU, [rows, tb_stride]) against float64"""
    lay, tb_cols, c0, c0p = tower_layout(sd32)
    assert got.shape[1] == tb_cols + 9 * c0p
    assert torch.isfinite(got).all(), what
    _, proj = ref64.time_tower(sd64, freqs, t, cond, present)
    _, bound = ref64.time_tower_bound(sd64, freqs, t, cond, present)
    g = got.double()
    for name, off, cout, cp in lay:
        err, S = (g[:, off: off + cout] - proj[name]).abs(), bound[name]
        ratio = (err / S.clamp_min(1e-300)).max().item() / U
        print(f"{what} {name}: max err / S = {ratio:.3f} * 2^-24")
        stats[("tower projected", sf)] = max(stats[("tower projected", sf)], ratio)
        assert (err <= C_T * U * S).all(), f"{what} {name}: max err / S = {ratio:.2f} * 2^-24 > {C_T}"
        assert not got[:, off + cout: off + cp].any(), f"{what} {name}: nonzero padding columns"
    want, S = ref64.class_biases(sd64["enc1.conv2.weight"], g[:, :c0])      # from the device's own enc1 columns
    cls = g[:, tb_cols:].reshape(-1, 9, c0p)
    err = (cls[:, :, :c0] - want).abs()
    ratio = (err / S.clamp_min(1e-300)).max().item() / U
    print(f"{what} class biases: max err / S = {ratio:.3f} * 2^-24")
    stats[("tower class-bias", sf)] = max(stats[("tower class-bias", sf)], ratio)
    assert (err <= C_B * U * S).all(), f"{what} class biases: max err / S = {ratio:.2f} * 2^-24 > {C_B}"
    assert not cls[:, :, c0:].any(), f"{what}: nonzero padding columns in a class vector"


@pytest.mark.parametrize("sf", TOWER_SF)
def test_time_tower_every_row_of_every_regime_vs_float64(sf, handles, cpu_threads, stats):
    h, sd32 = handles(sf)
    sd64 = {k: v.double() for k, v in sd32.items()}
    D = h.temb_dim
    assert D == max(int(256 * sf), 16)
    freqs = engine.sinusoid_frequencies(D)          # the table the handle was created with
    t, cond, present = tower_rows()
    t_d, c_d = i32(t), torch.tensor(cond, dtype=torch.float32, device=DEV)
    p_d = torch.tensor(present, dtype=torch.uint8, device=DEV)
    assert 0 < sum(present) < N_ROWS

    # every row on its own: one-row calls run the 8-slice form with a single row
    single = torch.cat([tower_call(h, t_d[r: r + 1], c_d[r: r + 1], p_d[r: r + 1], 1, POISONS[r % 2]) for r in range(N_ROWS)])
    for n in ROW_COUNTS:
        outs = [tower_call(h, t_d, c_d, p_d, n, v) for v in POISONS]
        assert torch.equal(bits(outs[0]), bits(outs[1])), f"sf {sf}, {n} rows: the output depends on what the buffer held"
        differ = (bits(outs[0]) != bits(single[:n])).any(dim=1).nonzero().flatten().tolist()
        assert not differ, f"sf {sf}, {n} rows: rows {differ[:8]} differ from one-row calls of the same (t, cond, present)"
        check_tower(outs[0].cpu(), sd32, sd64, freqs, t[:n], cond[:n], present[:n], f"sf {sf}, {n} rows", stats, sf)

    # a null cond: no row has a condition, whatever present says; a null present: every row has one
    n = N_ROWS
    for c_arg, p_arg, ref_c, ref_p, what in ((None, p_d, None, None, "null cond"), (c_d, None, cond, None, "null present")):
        outs = [tower_call(h, t_d, c_arg, p_arg, n, v) for v in POISONS]
        assert torch.equal(bits(outs[0]), bits(outs[1])), f"sf {sf}, {what}"
        check_tower(outs[0].cpu(), sd32, sd64, freqs, t, ref_c, ref_p, f"sf {sf}, {what}", stats, sf)
        same = torch.tensor([p == (0 if c_arg is None else 1) for p in present])
        assert torch.equal(bits(outs[0])[same.to(DEV)], bits(single)[same.to(DEV)]), f"sf {sf}, {what}: rows that mean the same differ"

    # the wrapper's three modes are the general form with the matching tensors (a condition value on a row without one is ignored)
    modes = [(COND_NONE, COND_ZERO, COND_ONE)[(r + r // 3) % 3] for r in range(70)]
    via_modes = h.time_bias(t[:70], modes)
    c_m = torch.tensor([{COND_NONE: 7.5, COND_ZERO: 0.0, COND_ONE: 1.0}[m] for m in modes], dtype=torch.float32, device=DEV)
    p_m = torch.tensor([m != COND_NONE for m in modes], dtype=torch.uint8, device=DEV)
    assert torch.equal(bits(via_modes), bits(h.time_bias_general(t_d[:70].contiguous(), c_m, p_m, 70))), f"sf {sf}: time_bias wrapper"


# ------------------------------------------------------------------ b. head
HEAD_SF = (0.05, 0.2, 0.3, 0.5, 1.0)        # c_real = 16 (half of a group's lanes idle), 25 (no multiple of 4), 38, 64, 128
HEAD_SHAPES = [(H, W, n_pass, B) for H, W in ((16, 16), (16, 48), (48, 16)) for n_pass in (1, 2) for B in (1, 5, 41)]


def head_case(h, sd32, H, W, n_pass, B, tb_div, seed, what, stats, key):
    C = h.channels
    rows = n_pass * B
    rng = random.Random(seed)
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)
    n_tb = rows // tb_div
    tb = h.time_bias([rng.randrange(1000) for _ in range(n_tb)], [rng.choice((COND_NONE, COND_ZERO, COND_ONE)) for _ in range(n_tb)])
    ws = h.workspace(rows, H, W)
    eps = torch.empty(rows, C, H, W, dtype=torch.float32, device=DEV)
    h.ensure_plan(rows, H, W, B, 0, tune=False)
    outs = []
    for value in POISONS:
        ws.view(torch.float32).fill_(value)
        eps.fill_(value)
        with torch.cuda.device(DEV):
            check(h.lib.dt_unet_forward(h.h, ptr(x), B, n_pass, H, W, ptr(tb), tb_div, ptr(eps), ptr(ws), c_size_t(ws.numel()),
                                        stream_ptr()), "dt_unet_forward")
        outs.append((eps.clone(), h.debug_activation(rows, H, W, 7).clone()))
    assert torch.equal(bits(outs[0][1]), bits(outs[1][1])), f"{what}: dec1 differs between the poisons"
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])), f"{what}: eps differs between NaN- and 1e30-poisoned workspaces"
    assert torch.isfinite(outs[0][0]).all(), f"{what}: eps is not finite"
    w, b = sd32["final.weight"], sd32["final.bias"]
    c_real = w.shape[1]
    dec1 = outs[0][1]
    assert dec1.shape[:3] == (rows, H // 2, W // 2) and dec1.shape[3] >= c_real
    d1 = dec1[..., :c_real].permute(0, 3, 1, 2).double().cpu()
    ref, S = ref64.head(d1, w.double(), b.double())
    got = outs[0][0].double().cpu()
    err = (got - ref).abs()
    ratio = (err / S.clamp_min(1e-300)).max().item() / U
    rel = ((got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1).clamp_min(1e-300)).max().item()
    print(f"{what}: max err / S = {ratio:.3f} * 2^-24, worst per-image relative L2 {rel:.3e}")
    stats[("head err/S" + key[0], key[1])] = max(stats[("head err/S" + key[0], key[1])], ratio)
    stats[("head rel L2" + key[0], key[1])] = max(stats[("head rel L2" + key[0], key[1])], rel)
    # the same with the interpolation weights as fp32 forms them (bilinear_src): what is left is the rounding of the sums
    ref32, S32 = ref64.head(d1, w.double(), b.double(), coord32=True)
    err32 = (got - ref32).abs()
    ratio32 = (err32 / S32.clamp_min(1e-300)).max().item() / U
    print(f"{what}: with fp32 interpolation weights, max err / S = {ratio32:.3f} * 2^-24")
    stats[("head, fp32 weights, err/S" + key[0], key[1])] = max(stats[("head, fp32 weights, err/S" + key[0], key[1])], ratio32)
    assert (err <= C_H * U * S).all(), f"{what}: max err / S = {ratio:.2f} * 2^-24 > {C_H}"
    assert rel <= REL_H, f"{what}: per-image relative L2 error {rel:.3e} > {REL_H:.0e}"
    assert (err32 <= C_HW * U * S32).all(), f"{what}: with fp32 interpolation weights, max err / S = {ratio32:.2f} * 2^-24 > {C_HW}"


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("sf", HEAD_SF)
def test_head_vs_float64_from_the_devices_dec1(sf, channels, handles, cpu_threads, stats):
    h, sd32 = handles(sf, channels, "head")
    assert not h.fused_active(16, 16) and h.channels == channels
    for i, (H, W, n_pass, B) in enumerate(HEAD_SHAPES):
        head_case(h, sd32, H, W, n_pass, B, 1, 100 * channels + i, f"sf {sf} C {channels} {H}x{W} B {B} x {n_pass}", stats, ("", sf))


def test_head_grid_wraps_beyond_262144_low_resolution_pixels(handles, cpu_threads, stats):
    """344 rows of 64 x 64: 352256 low-resolution pixels in groups of 32 are 11008 workgroups' worth for a grid of 8192"""
    h, sd32 = handles(0.05, 3, "head")
    assert 344 * 32 * 32 > 8192 * 32
    head_case(h, sd32, 64, 64, 2, 172, 172, 7, "sf 0.05 C 3 64x64 B 172 x 2", stats, (" (large case)", 0.05))


# ------------------------------------------------------------------ c. the interpolating update
class Step:
    """one sampler step of a batch: B images of which the first b_single take one pass (mixed batch), the others n_pass"""

    def __init__(self, name, B, n_pass=1, b_single=0, w=None, w_scalar=1.0, masked=False, noise=True):
        self.name, self.B, self.n_pass, self.b_single, self.w, self.w_scalar = name, B, n_pass, b_single, w, w_scalar
        self.masked, self.noise = masked, noise
        self.rows = n_pass * B - b_single * (n_pass - 1)
        self.tb_div = 1 if b_single else B          # a mixed batch has a time-bias row per batch row
        self.tb_rows = self.rows // self.tb_div


# per-image scales with 0 and 20 among the two-pass images; the one-pass images of a mixed batch (the first 1 or 3 of 7) carry
# scales other than 0 and 1, which an update that mixed them would show
W5, W7 = (0.0, 20.0, 1.5, 3.0, 7.5), (2.0, 5.0, 0.5, 0.0, 20.0, 1.5, 3.0)
STEPS = (
    Step("one pass", 5),
    Step("one pass, no noise", 5, noise=False),
    Step("two passes, w_scalar", 5, 2, w_scalar=3.7),
    Step("two passes, per-row w", 5, 2, w=W5),
    Step("mixed 1 of 7", 7, 2, 1, w=W7),
    Step("mixed 3 of 7", 7, 2, 3, w=W7),
    Step("masked, one pass", 5, masked=True),
    Step("masked, two passes, per-row w", 5, 2, w=W5, masked=True),
    Step("masked, mixed 3 of 7", 7, 2, 3, w=W7, masked=True),
)
Z_ROWS = 16
COEF = {RULE_ENGINE: (1.02, 0.07, 0.05), RULE_PSAMPLE: (1.01, 0.03, 0.02), RULE_MANAGER: (0.1, 0.95, 0.02)}


class StepData:
    """inputs of a step on the device: x0, the noise table with its row table, mask / known tables with theirs, tb rows"""

    def __init__(self, h, st, H, W, seed, n_steps=1):
        g = torch.Generator().manual_seed(seed)
        rng = random.Random(seed)
        B, E = st.B, h.channels * H * W
        self.E = E
        self.x0 = torch.randn(B, E, generator=g).to(DEV)
        self.z = torch.randn(Z_ROWS, E, generator=g).to(DEV)
        zr = [rng.randrange(6) for _ in range(B)]
        zr[2] = zr[0]                                   # a permutation with a repeat
        self.z_row = i32(zr)
        self.w = None if st.w is None else torch.tensor(st.w, dtype=torch.float32, device=DEV)
        self.mask = self.known = self.mask_row = self.known_row = None
        if st.masked:
            self.mask = torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (3, E), generator=g)].to(DEV)
            self.known = torch.randn(4, E, generator=g).to(DEV)
            self.mask_row = i32([rng.randrange(3) for _ in range(B)])
            self.known_row = i32([rng.randrange(4) for _ in range(B)])
        n = n_steps * st.tb_rows
        self.tb = h.time_bias([rng.randrange(1, 1000) for _ in range(n)], [rng.choice((COND_NONE, COND_ZERO, COND_ONE)) for _ in range(n)])


def sampler_steps(h, rule, st, d, H, W, x, tb, coef, noise, z_shift):
    """len(coef) steps of the layered sampler from x [B, E]; returns the trajectory [n + 1, B, E]"""
    n = len(coef)
    traj = torch.full((n + 1, st.B, d.E), float("nan"), device=DEV)
    traj[0] = x
    if st.masked:
        h.sample_masked(rule, traj, H, W, tb, st.n_pass, coef, noise, d.mask, d.known, d.mask_row, d.known_row, z=d.z, z_row=d.z_row,
                        z_shift=z_shift, w=d.w, w_scalar=st.w_scalar, b_single=st.b_single, tb_div=st.tb_div)
    elif st.b_single:
        h.sample_mixed(rule, traj, H, W, tb, st.tb_div, st.b_single, coef, noise, d.z, d.z_row, z_shift, d.w)
    else:
        h.sample(rule, traj, H, W, tb, st.n_pass, coef, noise, z=d.z, z_row=d.z_row, z_shift=z_shift, w=d.w, w_scalar=st.w_scalar)
    return traj


def forward_plus_flat_update(h, rule, st, d, H, W, x, tb, coef, noise, z_shift):
    """the same step from its parts: the forward's eps, then dt_cfg_update(_masked) on the flat predictions; the rows of a mixed
    batch that take one pass are updated without a second prediction, the others with eps[B:]"""
    B = st.B
    x4 = x.reshape(B, h.channels, H, W)
    eps = h.forward_mixed(x4, tb, st.b_single, st.tb_div) if st.b_single else h.forward(x4, tb, st.n_pass, st.tb_div)
    assert eps.shape[0] == st.rows
    zg = d.z[d.z_row.long() + z_shift] if noise else None
    parts = ([(0, st.b_single, None)] if st.b_single else []) + [(st.b_single, B, eps[B:] if st.n_pass == 2 else None)]
    out = []
    for lo, hi, ec in parts:
        args = (rule, x[lo:hi], eps[lo:hi], ec, None if zg is None else zg[lo:hi].contiguous(), coef, noise)
        kw = dict(w=None if d.w is None or ec is None else d.w[lo:hi], w_scalar=st.w_scalar)
        if st.masked:
            out.append(engine.cfg_update_masked(*args, d.mask, d.known, d.mask_row[lo:hi], d.known_row[lo:hi], **kw))
        else:
            out.append(engine.cfg_update(*args, **kw))
    return torch.cat(out)


@pytest.mark.parametrize("H,W", [(16, 48), (48, 16), (32, 16)])
@pytest.mark.parametrize("sf", [0.2, 0.5])
def test_layered_step_is_forward_plus_flat_update(sf, H, W, handles):
    h, _ = handles(sf, 3, "layered")
    assert not h.fused_active(H, W)
    failures = []
    for si, st in enumerate(STEPS):
        for rule in RULES:
            d = StepData(h, st, H, W, 1000 * si + rule)
            z_shift = 2 + rule
            got = sampler_steps(h, rule, st, d, H, W, d.x0, d.tb, [COEF[rule]], [st.noise], [z_shift])
            want = forward_plus_flat_update(h, rule, st, d, H, W, d.x0, d.tb, COEF[rule], st.noise, z_shift)
            assert torch.equal(got[0], d.x0)
            if rule == RULE_ENGINE and not st.noise:
                want = d.x0                                # the dead step records x unchanged
            if not torch.equal(bits(got[1]), bits(want)):
                bad = (bits(got[1]) != bits(want)).any(dim=1).nonzero().flatten().tolist()
                failures.append(f"{st.name}, rule {rule}: rows {bad} differ, max |diff| {(got[1] - want).abs().max().item():.3e}")
    assert not failures, f"sf {sf} {H}x{W}: {len(failures)} steps differ from forward + flat update:\n  " + "\n  ".join(failures)


@pytest.mark.parametrize("H,W", [(16, 48), (32, 16)])
def test_engine_dead_step_copies_x_and_runs_no_forward(H, W, handles):
    h, _ = handles(0.2, 3, "layered")
    st = Step("two passes", 5, 2, w_scalar=3.7)
    d = StepData(h, st, H, W, 77)
    h.forward(d.x0.reshape(st.B, 3, H, W), d.tb, 2, st.B)      # settles the shape's plan: the loop then runs no forward of its own
    ws = h.workspace(st.rows, H, W)
    for value in POISONS:
        ws.view(torch.float32).fill_(value)
        before = ws.clone()
        got = sampler_steps(h, RULE_ENGINE, st, d, H, W, d.x0, d.tb, [COEF[RULE_ENGINE]], [False], [3])
        assert torch.equal(bits(got[1]), bits(d.x0)) and torch.equal(bits(got[0]), bits(d.x0))
        assert torch.equal(ws, before), "the dead step wrote to the workspace"


def test_update_and_head_grids_wrap_on_a_large_step(handles):
    """172 images of 64 x 64, two passes: 528384 quads for the update's 2048 workgroups of 256 threads (524288), and 352256
    low-resolution pixels for the head"""
    h, _ = handles(0.05, 3, "layered")
    H = W = 64
    st = Step("two passes, w_scalar", 172, 2, w_scalar=2.5)
    assert st.B * 3 * H * W // 4 > 2048 * 256
    d = StepData(h, st, H, W, 5)
    rule = RULE_PSAMPLE
    got = sampler_steps(h, rule, st, d, H, W, d.x0, d.tb, [COEF[rule]], [True], [4])
    want = forward_plus_flat_update(h, rule, st, d, H, W, d.x0, d.tb, COEF[rule], True, 4)
    bad = (bits(got[1]) != bits(want)).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"rows {bad[:10]} differ from forward + flat update"


@pytest.mark.parametrize("step", [STEPS[2], STEPS[5], STEPS[7]], ids=["two-passes", "mixed-3-of-7", "masked-two-passes"])
def test_three_step_loop_is_three_chained_one_step_loops(step, handles):
    """slot i + 1 is step i's output and step i + 1's input; step i reads its own time-bias rows, coefficients and z_shift"""
    h, _ = handles(0.2, 3, "layered")
    H, W, st = 16, 48, step
    for rule, noise in ((RULE_ENGINE, [True, True, False]), (RULE_PSAMPLE, [True, True, False]), (RULE_MANAGER, [True, True, True])):
        d = StepData(h, st, H, W, 31 + rule, n_steps=3)
        coef = [tuple(c * (1.0 + 0.25 * i) for c in COEF[rule]) for i in range(3)]
        z_shift = [0, 7, 3]
        full = sampler_steps(h, rule, st, d, H, W, d.x0, d.tb, coef, noise, z_shift)
        assert torch.isfinite(full).all()
        x = d.x0
        for i in range(3):
            tb_i = d.tb[i * st.tb_rows: (i + 1) * st.tb_rows]
            one = sampler_steps(h, rule, st, d, H, W, x, tb_i, [coef[i]], [noise[i]], [z_shift[i]])
            assert torch.equal(bits(one[1]), bits(full[i + 1])), f"{st.name}, rule {rule}: step {i} of the loop differs from a one-step loop"
            x = one[1].clone()
        assert not torch.equal(full[1], full[2])
