"""Every convolution launch choice, one U-Net block at a time, against a float64 evaluation of that block.

For block j the test pins one of its convolutions (slot 0 skip, 1 conv1, 2 conv2) through dt_unet_set_conv_choice, runs the
forward and reads block j's output (dt_unet_debug_activation, head fusion off so that every block output is stored).  Blocks
upstream of j keep their own launches, so j's input is what the heuristic plan computed -- checked bit for bit -- and j's
float64 reference is computed once per case from that input:

  * elementwise  |got - ref64| <= TAU * S, S the same block evaluated on |input| with every weight, bias, folded-BN
    scale / shift and time-bias term replaced by its magnitude (the sum of the terms' magnitudes at each stage);
  * per image    relative L2 error against float64 <= REL_L2, and the RMS of err / S <= RMS_C * 2^-24, for every batch row
    on its own (tail rows of a ragged tile cannot hide in an average);
  * padding      channels cout .. cout_p of the block output are exactly 0;
  * poisoning    the workspace and eps are filled with NaN, then with 1e30, before the forward: the block output and eps
    must come out bit-identical (no launch reads an element that no launch of the forward wrote) and eps finite.

The cases cover the ragged M tiles of 41 images (4x4 / 2x2 / 1x1 levels), the 256 x 64 tiles and the epilogue modes of the
half-size model, odd channel counts (38 / 51 channels), 32 x 32 pictures (2 x 2 bottleneck), a mixed batch (shared enc1 with
single-pass images) and a one-pass forward (a pin keyed by the one-pass image split); and five rectangular pictures whose
level widths are no power of two (cases G .. K, see CASES), where no tile height is a multiple of the width: every strip
tile starts and ends inside a picture row and takes the halo W + 1 (strip_halo), rows and columns are told apart, the
bottleneck is a 1 x 3 or a 3 x 1 picture that walks nine taps, a width of 56 puts the K = 32 forms 256 x 64 and 128 x 128 at their
LDS limit of 98 304 B (48 px: 95 232 B), and levels of 112 / 80 pixels fall back to the GEMM kinds.

  case                        H x W    B   admissible  run   refused at launch (stripk 64 x 64 on rows > 31 px)
  A_sf1.0_16px_B41           16 x 16  41      1472     1472  -
  B_sf0.5_16px_B41           16 x 16  41      1253     1253  -
  C_sf0.3_16px_B41           16 x 16  41       996      996  -
  C_sf0.4_16px_B41           16 x 16  41       970      970  -
  D_sf1.0_32px_B5            32 x 32   5      1606     1605  enc1.conv2 (32 px)
  E_sf0.5_mixed_B9_single3   16 x 16   9+6    1253     1253  -
  F_sf0.5_one_pass_B12       16 x 16  12      1253     1253  -
  G_sf0.5_16x48_B5           16 x 48   5      1371     1370  enc1.conv2 (48 px)
  H_sf0.5_48x16_B5           48 x 16   5      1371     1371  -
  I_sf0.5_16x112_B2          16 x 112  2      1363     1354  enc2 and dec1 (56 px), 9 launches
  J_sf0.3_32x48_B3           32 x 48   3      1138     1137  enc1.conv2 (48 px)
  K_sf1.0_16x80_B3           16 x 80   3      1593     1580  enc2 and dec1 (40 px), 13 launches

(min_launches is that count rounded down.)  On G, H and J the strip kinds 3 / 4 / 5 ran on every 3x3 slot with every
tile the channel count admits (kind 5's 64 x 64 tile up to 31 px); on I's 56 px levels kind 4 ran 256 x 64, 128 x 128, 128 x 64,
64 x 128 and 64 x 64 -- nothing is refused at 56, 48 or 40 px but stripk 64 x 64.

What a pinned conv2 launch writes besides its block output:

  * head fusion on, for every dec1.conv2 pin: eps agrees with the head-off eps of the same pin to REL_L2 per row and is
    bit-identical under both poisons; dec1's output is left unwritten exactly where the rule fuses the head (one N tile, no
    split).  For every enc1.conv2 pin: enc2's output is bit-identical to the head-off run of the same pin, and enc1's own
    output is left unwritten exactly where its epilogue pools (skip_out);
  * test_pinned_conv2_launches_write_the_max_pool: the 2x2 max pool behind enc1 .. enc4, written by conv2's staged epilogue,
    by the slab sum of a split launch or by maxpool_kernel, read back exactly through a transparent next block.

Every case runs every launch the rules admit (about 15600 in all, twice each, the 880 pool pins and the 920 head-fusion
reruns aside): on one MI355X the module takes about 26 s (16 s before cases G .. K and the pool test; each new case 1.6 to
2.8 s, each pool shape 0.3 to 0.4 s).
"""
import math
import random
from collections import defaultdict
from ctypes import byref, c_int, c_size_t
from typing import NamedTuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd._hip import COND_NONE, COND_ONE, COND_ZERO, HipLibraryError, check, ptr, stream_ptr
from fused_readout import transparent    # block j as an exact selection of its input (tests/fused_readout.py)
from oracle import unet_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# Elementwise bound TAU * S with TAU = C_TAU * 2^-24.  Measured on an MI355X over every launch of every case: max err / S
# = 0.50 * 2^-24 (fp32 0.42, split-bf16 0.50, strip 0.47, strip32 0.44, stripk 0.40); C_TAU keeps a 4x margin.  The
# rectangular cases G .. K alone: 0.42 (fp32 0.37, split-bf16 0.41, strip 0.42, strip32 0.42, stripk 0.31) -- an output
# element's fma chain is as long on any picture shape, out-of-picture taps add nothing
C_TAU = 2
TAU = C_TAU * 2.0 ** -24
REL_L2 = 1e-6                    # per-image relative L2 error of a block output against float64 (measured max 5.2e-7; G .. K 5.0e-7)
# per-image RMS of err / S, in units of 2^-24: measured max 0.096 (fp32, split-bf16 GEMM kinds), 0.045 (strip kinds); on
# G .. K 0.033 (fp32), 0.036 (split-bf16 and the strip kinds).  Far below the elementwise bound, it sees errors the size of
# fp32 rounding spread over a whole image, e.g. one of the six plane products of a strip kind dropped (0.29)
RMS_C = 0.2
POISONS = (float("nan"), 1e30)   # fmaxf-style ReLUs turn a NaN read into 0: a large finite value is needed too
KDIV = (1, 2, 4, 8, 16, 8, 4, 2)
SLOT_NAMES = ("skip", "conv1", "conv2")
AXES = dict(bm=(64, 128, 256), bn=(64, 128), splits=range(1, 10), kind=range(6), fuse=(0, 1))   # record_launch_rules.GRID_AXES
SKIP_CONV2 = (64, 64, 1, 1, 0)   # conv2 pinned unfused while the 1x1 skip runs as a launch of its own


class Case(NamedTuple):
    name: str
    sf: float
    H: int
    W: int
    B: int
    n_pass: int
    single: int      # single-pass images of a mixed batch (dt_unet_forward_mixed)
    tb_div: int
    min_launches: int   # distinct launches the rules admit (at least)
    seed: int


CASES = (
    Case("A_sf1.0_16px_B41", 1.0, 16, 16, 41, 2, 0, 41, 1400, 1),
    Case("B_sf0.5_16px_B41", 0.5, 16, 16, 41, 2, 0, 1, 1200, 2),
    Case("C_sf0.3_16px_B41", 0.3, 16, 16, 41, 2, 0, 1, 950, 3),
    Case("C_sf0.4_16px_B41", 0.4, 16, 16, 41, 2, 0, 1, 920, 4),
    Case("D_sf1.0_32px_B5", 1.0, 32, 32, 5, 2, 0, 1, 1500, 5),
    Case("E_sf0.5_mixed_B9_single3", 0.5, 16, 16, 9, 2, 3, 1, 1200, 6),
    Case("F_sf0.5_one_pass_B12", 0.5, 16, 16, 12, 1, 0, 1, 1200, 7),
    # rectangular pictures: no tile height is a multiple of the level width, so every strip tile takes the halo W + 1
    Case("G_sf0.5_16x48_B5", 0.5, 16, 48, 5, 2, 0, 1, 1350, 8),      # rows of 48 .. 3 px; the bottleneck is 1 x 3 (nine taps)
    Case("H_sf0.5_48x16_B5", 0.5, 48, 16, 5, 2, 0, 1, 1350, 9),      # heights 48 .. 3 on widths 16 .. 1; the bottleneck is 3 x 1
    Case("I_sf0.5_16x112_B2", 0.5, 16, 112, 2, 2, 0, 1, 1350, 10),   # 112 px: GEMM kinds only; 56 px: strip forms at their LDS limit
    Case("J_sf0.3_32x48_B3", 0.3, 32, 48, 3, 2, 0, 1, 1100, 11),     # 38 / 76 channels with the halo W + 1
    Case("K_sf1.0_16x80_B3", 1.0, 16, 80, 3, 2, 0, 1, 1550, 12),     # bn = 128 forms; 80 px GEMM only, 40 px without stripk 64 x 64
)


@pytest.fixture(scope="module")
def cpu_threads():
    """float64 references on at most 16 threads (a GPU box may show many more cores than a job may use)"""
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(old, 16)))
    yield
    torch.set_num_threads(old)


@pytest.fixture(scope="module")
def stats():
    """per launch kind: the largest err / S (in units of 2^-24), per-image relative L2 error and per-image RMS of err / S"""
    table = defaultdict(lambda: [0.0, 0.0, 0.0, 0])
    yield table
    print("\nper-kind maxima over all cases: kind: (max err/S [2^-24], max per-image rel L2, max per-image RMS err/S [2^-24], "
          "variants)")
    for kind in sorted(table):
        r, l2, rms, n = table[kind]
        print(f"  {_hip.KIND_NAMES.get(kind, kind)}: ({r:.3f}, {l2:.3e}, {rms:.4f}, {n})")


# ------------------------------------------------------------------ batch rows of a case
def row_images(c):
    """image of every batch row: [pass 0 of all images | passes 1.. of images single..B-1]"""
    return list(range(c.B)) + [b for _ in range(c.n_pass - 1) for b in range(c.single, c.B)]


def row_conditions(c):
    """(t, cond mode) of every time-bias row (row r of the batch uses tb row r // tb_div)"""
    rows = len(row_images(c)) // c.tb_div
    rng = random.Random(100 + c.seed)
    if c.tb_div == c.B:     # one row per pass, the sampler's CFG layout
        return [(9, COND_NONE), (9, COND_ONE)][:rows]
    modes = (COND_NONE, COND_ZERO, COND_ONE)
    return [(rng.randrange(0, 1000), modes[rng.randrange(3)]) for _ in range(rows)]


def row_temb(sd32, conds, tb_div):
    """float64 [rows, D] time embedding of every batch row, evaluated in fp32 as the device's time-bias kernel does"""
    t = torch.tensor([tc[0] for tc in conds], dtype=torch.long)
    embs = {COND_NONE: unet_ref.time_embedding(sd32, t, None),
            COND_ZERO: unet_ref.time_embedding(sd32, t, torch.zeros(len(conds), 1)),
            COND_ONE: unet_ref.time_embedding(sd32, t, torch.ones(len(conds), 1))}
    temb = torch.stack([embs[m][i] for i, (_, m) in enumerate(conds)]).double()
    return temb.repeat_interleave(tb_div, dim=0)


# ------------------------------------------------------------------ float64 block and its magnitude bound
def _folded_bn(sd, name, i):
    """(scale, magnitude of the folded shift) of conv i + BatchNorm: y = scale * conv + ((bias - mean) * scale + beta)"""
    scale = sd[f"{name}.norm{i}.weight"] / torch.sqrt(sd[f"{name}.norm{i}.running_var"] + 1e-5)
    mag = (sd[f"{name}.conv{i}.bias"].abs() + sd[f"{name}.norm{i}.running_mean"].abs()) * scale.abs() + sd[f"{name}.norm{i}.bias"].abs()
    return scale.abs()[None, :, None, None], mag[None, :, None, None]


def block_bound(sd, name, xa, temb):
    """S: models.py's Block on the input magnitudes xa with every term replaced by its magnitude"""
    s1, a1 = _folded_bn(sd, name, 1)
    h = s1 * F.conv2d(xa, sd[name + ".conv1.weight"].abs(), padding=1) + a1
    h = h + F.linear(temb.abs(), sd[name + ".time_mlp.weight"].abs(), sd[name + ".time_mlp.bias"].abs())[:, :, None, None]
    s2, a2 = _folded_bn(sd, name, 2)
    out = s2 * F.conv2d(h, sd[name + ".conv2.weight"].abs(), padding=1) + a2
    rkey = name + ".residual_conv.weight"
    return out + (F.conv2d(xa, sd[rkey].abs(), sd[name + ".residual_conv.bias"].abs()) if rkey in sd else xa)


def _up(a):
    return F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=True)


def block_references(sd64, x64, acts, temb):
    """{j: (ref64, S)} of every block, from the device's own outputs of the blocks upstream (acts: float64 NCHW)"""
    out = {}
    with torch.no_grad():
        for j, name in enumerate(engine.BLOCK_NAMES):
            if j == 0:
                xin, xa = x64, x64.abs()
            elif j <= 4:
                xin = F.max_pool2d(acts[j - 1], 2)
                xa = xin.abs()
            else:
                prev, skip = acts[j - 1], acts[8 - j]
                xin = torch.cat([_up(prev), skip], 1)
                xa = torch.cat([_up(prev.abs()), skip.abs()], 1)    # bilinear terms summed by magnitude
            out[j] = (unet_ref.block_forward(sd64, name, xin, temb), block_bound(sd64, name, xa, temb))
    return out


# ------------------------------------------------------------------ one case on the device
class Runner:
    def __init__(self, c, sd32):
        self.c = c
        self.h = engine.UNetHandle(sd32, DEV)
        self.h.set_head_fusion(False)
        self.h.set_fused(False)
        self.imgs = row_images(c)
        self.rows = len(self.imgs)
        g = torch.Generator().manual_seed(1000 + c.seed)
        self.x = torch.randn(c.B, 3, c.H, c.W, generator=g)
        self.x_dev = self.x.to(DEV)
        self.conds = row_conditions(c)
        self.tb = self.h.time_bias([t for t, _ in self.conds], [m for _, m in self.conds])
        self.ws = self.h.workspace(self.rows, c.H, c.W)
        self.eps = torch.empty(self.rows, 3, c.H, c.W, dtype=torch.float32, device=DEV)
        self.couts = [sd32[f"{n}.conv2.weight"].shape[0] for n in engine.BLOCK_NAMES]

    # -- library calls
    def forward(self):
        """one forward into self.eps / the workspace; returns the library status"""
        c, h = self.c, self.h
        with torch.cuda.device(DEV):
            if c.single:
                return h.lib.dt_unet_forward_mixed(h.h, ptr(self.x_dev), c.B, c.single, c.H, c.W, ptr(self.tb), c.tb_div,
                                                   ptr(self.eps), ptr(self.ws), c_size_t(self.ws.numel()), stream_ptr())
            return h.lib.dt_unet_forward(h.h, ptr(self.x_dev), c.B, c.n_pass, c.H, c.W, ptr(self.tb), c.tb_div, ptr(self.eps),
                                         ptr(self.ws), c_size_t(self.ws.numel()), stream_ptr())

    def poisoned_forward(self, value):
        self.ws.view(torch.float32).fill_(value)
        self.eps.fill_(value)
        return self.forward()

    def act(self, j):
        return self.h.debug_activation(self.rows, self.c.H, self.c.W, j)

    def report(self, j, slot, split=None):
        """dt_unet_conv_choice's report for the case's own shape, or for another (images, single-pass images) of its rows"""
        v = [c_int() for _ in range(5)]
        imgs, single = split or (self.c.B, self.c.single)
        check(self.h.lib.dt_unet_conv_choice(self.h.h, self.rows, self.c.H, self.c.W, imgs, single, j, slot, *map(byref, v)), "dt_unet_conv_choice")
        return tuple(x.value for x in v)

    def pin(self, j, slot, bm, bn, splits, kind, fuse):
        """fresh heuristic plan + one pinned slot (slot 0: conv2 pinned unfused first); False where the library refuses"""
        h, c = self.h, self.c
        h.set_precision(_hip.PREC_AUTO)
        try:
            if slot == 0:
                h.set_conv_choice(self.rows, c.H, c.W, j, 2, *SKIP_CONV2, images=c.B, single=c.single)
            h.set_conv_choice(self.rows, c.H, c.W, j, slot, bm, bn, splits, kind, fuse, images=c.B, single=c.single)
        except HipLibraryError:
            return False
        return True

    # -- the launch vocabulary
    def admissible(self, blocks=range(8), slots=range(3)):
        """{(j, slot, resolved report [bm, bn, splits, kind + 8 fuse]): request} over the whole vocabulary"""
        found = {}
        for j in blocks:
            for slot in slots:
                for bm in AXES["bm"]:
                    for bn in AXES["bn"]:
                        for sp in AXES["splits"]:
                            for kind in AXES["kind"]:
                                for fuse in AXES["fuse"]:
                                    if fuse and slot != 2:
                                        continue
                                    if not self.pin(j, slot, bm, bn, sp, kind, fuse):
                                        continue
                                    rep = self.report(j, slot)
                                    if rep[0] == 0:
                                        continue         # no launch of its own (enc1's first conv / skip, identity skips)
                                    found.setdefault((j, slot) + rep[:4], (bm, bn, sp, kind, fuse))
        self.h.set_precision(_hip.PREC_AUTO)
        return found


def level(c, j):
    """(height, width) of block j's pictures"""
    return c.H // KDIV[j], c.W // KDIV[j]


def expected_kinds(c, j, slot):
    """launch kinds the rules admit for a slot (resolve_conv_choice, conv_layer): the strip kinds need a full 3x3 walk -- not
    a 1x1 conv, and not a 1x1 picture, whose convolutions keep the centre tap only; a 1 x 3 or 3 x 1 picture walks all nine
    -- over picture rows of at most 63 pixels"""
    h, w = level(c, j)
    return {0, 1} if slot == 0 or (h == 1 and w == 1) or w > 63 else {0, 1, 3, 4, 5}


def check_block(got, ref, S, cout):
    """[any elementwise failure, max err/S, max per-image rel L2, any nonzero padding, max per-image RMS of err/S] as one
    device tensor"""
    g = got[..., :cout].permute(0, 3, 1, 2).double()
    err = (g - ref).abs()
    bad = ~(err <= TAU * S + 1e-30)
    q = torch.nan_to_num(err / S.clamp_min(1e-300), nan=math.inf)
    rel = torch.nan_to_num((g - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1).clamp_min(1e-300), nan=math.inf).amax()
    rms = q.flatten(1).square().mean(dim=1).sqrt().amax()
    pad = (got[..., cout:] != 0).any() if got.shape[-1] > cout else torch.zeros((), dtype=torch.bool, device=got.device)
    return torch.stack([bad.any().double(), q.amax(), rel, pad.double(), rms])


def bits(t):
    return t.contiguous().view(torch.int32)


def dec1_head_fuses(run, rep):
    """resolve_forward: dec1.conv2 evaluates the 1x1 head where its workgroups hold whole rows -- one N tile, no split"""
    return rep[2] == 1 and rep[1] == -(-run.couts[7] // 64) * 64


def enc1_pools_in_epilogue(c):
    """resolve_forward's pool rule for enc1.conv2 (never split): its staged epilogue pools where W is a power of two <= 16;
    with head fusion on, shared enc1 then stores the pool alone (skip_out)"""
    w = c.W
    return w <= 16 and w & (w - 1) == 0


def run_case(c, models, stats, log=None):
    """log: a list that receives (launch, [its failures]) of every launch run (tools)"""
    sd32 = {k: v.float() for k, v in models(c.sf).state_dict().items() if v.dtype.is_floating_point}
    sd64 = {k: v.double() for k, v in sd32.items()}
    run = Runner(c, sd32)
    h, rows = run.h, run.rows

    if c.name.startswith("F_"):
        # the pin of a one-pass shape made before its first forward is the one the forward runs (the library would otherwise
        # key it by the two-pass split images = rows / 2)
        ref_j, ref_slot = 2, 1
        h.set_conv_choice(rows, c.H, c.W, ref_j, ref_slot, 64, 64, 1, _hip.KIND_FP32, 0, images=c.B)
        h.forward(run.x_dev, run.tb, c.n_pass, c.tb_div)
        rep = run.report(ref_j, ref_slot)
        assert rep == (64, 64, 1, _hip.KIND_FP32, 1), f"pin before the first one-pass forward was dropped: report {rep}"
        assert set(h.plan_ids().values()) == {"pinned"}, h.plan_ids()
        # the pin belongs to that split alone: another split of the same rows (the two-pass one) settles a plan of its own
        other = h.ensure_plan(rows, c.H, c.W, rows // 2, 0)
        assert other != "pinned" and run.report(ref_j, ref_slot, (rows // 2, 0))[4] == 0, (other, h.plan_ids())
        assert h.ensure_plan(rows, c.H, c.W, c.B, c.single) == "pinned" and run.report(ref_j, ref_slot) == rep, h.plan_ids()
        h.set_precision(_hip.PREC_AUTO)            # drops the pins: the next forward settles its own plan
        h.forward(run.x_dev, run.tb, c.n_pass, c.tb_div)
        assert "pinned" not in h.plan_ids().values() and run.report(ref_j, ref_slot)[4] == 0, h.plan_ids()
    h.ensure_plan(rows, c.H, c.W, c.B, c.single, tune=False)

    # the heuristic plan's block outputs: the inputs of the references, and what every pinned forward must leave upstream
    h.set_precision(_hip.PREC_AUTO)
    base = []
    for value in POISONS:
        check(run.poisoned_forward(value), "dt_unet_forward")
        base.append(([run.act(j).clone() for j in range(8)], run.eps.clone()))
    for j in range(8):
        assert torch.equal(bits(base[0][0][j]), bits(base[1][0][j])), f"{c.name}: heuristic plan, {engine.BLOCK_NAMES[j]} reads unwritten memory"
    assert torch.equal(bits(base[0][1]), bits(base[1][1])) and torch.isfinite(base[0][1]).all(), f"{c.name}: heuristic plan, eps"
    acts = [a[..., :cout].permute(0, 3, 1, 2).double().cpu() for a, cout in zip(base[0][0], run.couts)]
    x64 = run.x.double()[run.imgs]
    temb = row_temb(sd32, run.conds, c.tb_div)
    refs = {j: (r.to(DEV), s.to(DEV)) for j, (r, s) in block_references(sd64, x64, acts, temb).items()}

    found = run.admissible()
    admitted = defaultdict(set)
    for key in found:
        admitted[key[:2]].add(key[5] & 7)
    for (j, slot), kinds in admitted.items():
        assert kinds == expected_kinds(c, j, slot), f"{c.name}: {engine.BLOCK_NAMES[j]}.{SLOT_NAMES[slot]} admits kinds {sorted(kinds)}"
    assert len(found) >= c.min_launches, f"{c.name}: the rules admit only {len(found)} distinct launches"

    failures, ran, refused, seen = [], 0, [], defaultdict(set)
    strip_ran, head_runs = defaultdict(set), [0, 0, 0, 0]   # [dec1.conv2 pins, with the head fused, enc1.conv2 pins, under skip_out]
    for key in [None] + sorted(found):
        n_before = len(failures)
        if key is None:                       # the heuristic plan itself
            j, slot, what = None, None, "heuristic plan"
            h.set_precision(_hip.PREC_AUTO)
        else:
            j, slot = key[:2]
            req = found[key]
            what = f"{engine.BLOCK_NAMES[j]}.{SLOT_NAMES[slot]} {_hip.KIND_NAMES[key[5] & 7]} {key[2]}x{key[3]} s{key[4]}" \
                   f"{' +skip' if key[5] & 8 else ''} (kind {key[5] & 7}, request {req})"
            assert run.pin(j, slot, *req), what
            assert run.report(j, slot)[:4] == key[2:], f"{what}: resolves differently on a second pin"
        outs, flags = [], []
        status = 0
        for value in POISONS:
            status = run.poisoned_forward(value)
            if status < 0:
                break
            check(status, f"dt_unet_forward ({what})")
            blocks = range(8) if j is None else [j]
            outs.append(([run.act(b).clone() for b in blocks], run.eps.clone()))
            if j == 0:
                next_off = run.act(1).clone()
            if j is not None:
                flags += [(bits(run.act(u)) != bits(base[0][0][u])).any() for u in range(j)]
        if status < 0:
            refused.append(key)               # the launcher refuses a choice the rules resolve to (e.g. its LDS or reach)
            continue
        if key is not None:
            rep = run.report(j, slot)
            if rep[:4] != key[2:] or rep[4] != 1:
                failures.append(f"{what}: the report after the forward shows {rep}, not the pin")
        ran += 1
        for b_idx, b in enumerate(range(8) if j is None else [j]):
            ref, S = refs[b]
            res = check_block(outs[0][0][b_idx], ref, S, run.couts[b])
            differs = (bits(outs[0][0][b_idx]) != bits(outs[1][0][b_idx])).any()
            bad, ratio, rel, pad, rms = res.tolist()
            kind = key[5] & 7 if key is not None else None
            where = what if key is not None else f"{what}, {engine.BLOCK_NAMES[b]}"
            if differs.item():
                failures.append(f"{where}: block output differs between NaN- and 1e30-poisoned workspaces")
            if bad:
                failures.append(f"{where}: |err| > {C_TAU} * 2^-24 * S (max err/S = {ratio * 2 ** 24:.2f} * 2^-24)")
            if rel > REL_L2:
                failures.append(f"{where}: per-image relative L2 error {rel:.3e} > {REL_L2:.0e}")
            if rms * 2 ** 24 > RMS_C:
                failures.append(f"{where}: per-image RMS of err/S {rms * 2 ** 24:.3f} * 2^-24 > {RMS_C} * 2^-24")
            if pad:
                failures.append(f"{where}: nonzero padding channels")
            if kind is not None:
                st = stats[kind]
                st[0], st[1], st[2], st[3] = max(st[0], ratio * 2 ** 24), max(st[1], rel), max(st[2], rms * 2 ** 24), st[3] + 1
                seen[(j, slot)].add(kind)
                if kind >= 3:
                    strip_ran[(level(c, j)[1], kind)].add(key[2:4])
        if not torch.equal(bits(outs[0][1]), bits(outs[1][1])) or not torch.isfinite(outs[0][1]).all():
            failures.append(f"{what}: eps differs between poisons or is not finite")
        if flags and torch.stack(flags).any().item():
            failures.append(f"{what}: a block upstream of the pinned one changed")
        if slot == 2 and j in (0, 7):
            # the same pin with head fusion on (the default).  dec1.conv2: its epilogue evaluates the 1x1 head where the rule
            # says so and dec1's output is then not stored; eps against the head-off eps of this pin.  enc1.conv2: it stores
            # the pool alone where its epilogue pools (skip_out); enc2's output is bit-identical to the head-off run of this pin
            h.set_head_fusion(True)
            on = []
            for value in POISONS:
                check(run.poisoned_forward(value), f"dt_unet_forward ({what}, head fusion on)")
                on.append((run.act(1).clone(), run.eps.clone(), torch.isnan(run.act(j)).all().item()))
            h.set_head_fusion(False)
            if not torch.equal(bits(on[0][1]), bits(on[1][1])) or not torch.isfinite(on[0][1]).all():
                failures.append(f"{what}: head fusion on, eps differs between poisons or is not finite")
            unstored = dec1_head_fuses(run, key[2:]) if j == 7 else enc1_pools_in_epilogue(c)
            if on[0][2] != unstored:         # (first poison: NaN)
                failures.append(f"{what}: head fusion on, the block output is {'not ' if on[0][2] else ''}stored")
            head_runs[0 if j == 7 else 2] += 1
            head_runs[1 if j == 7 else 3] += unstored
            if j == 7:
                e_on, e_off = on[0][1].double(), outs[0][1].double()
                rel_eps = ((e_on - e_off).flatten(1).norm(dim=1) / e_off.flatten(1).norm(dim=1)).max().item()
                if not rel_eps <= REL_L2:
                    failures.append(f"{what}: eps with head fusion on differs by {rel_eps:.3e} (relative L2, worst row)")
            elif not torch.equal(bits(on[0][0]), bits(next_off)):
                failures.append(f"{what}: head fusion on changes enc2's output")
        if log is not None:
            log.append((what, failures[n_before:]))

    # head fusion on (the default): the heuristic plan's stored block outputs are bit-identical to the head-off run, eps agrees
    h.set_head_fusion(True)
    h.set_precision(_hip.PREC_AUTO)
    fused = []
    for value in POISONS:
        check(run.poisoned_forward(value), "dt_unet_forward (head fusion on)")
        fused.append(([run.act(j).clone() for j in range(8)], run.eps.clone()))
    h.set_head_fusion(False)
    assert torch.equal(bits(fused[0][1]), bits(fused[1][1])) and torch.isfinite(fused[0][1]).all(), f"{c.name}: head fusion on, eps"
    for j in range(8):
        a = fused[0][0][j]
        if j in (0, 7) and torch.isnan(a).all():
            continue                           # not stored with head fusion on: enc1 under skip_out, dec1 under the fused head
        assert torch.equal(bits(a), bits(base[0][0][j])), f"{c.name}: head fusion on changes {engine.BLOCK_NAMES[j]}"
    e_on, e_off = fused[0][1].double(), base[0][1].double()
    rel_eps = ((e_on - e_off).flatten(1).norm(dim=1) / e_off.flatten(1).norm(dim=1)).max().item()
    assert rel_eps <= REL_L2, f"{c.name}: eps with the fused head differs by {rel_eps:.3e} (relative L2, worst row)"

    print(f"\n{c.name}: {len(found)} admissible launches, {ran - 1} run, refused at launch: {refused}, head-fused eps "
          f"{'bit-identical' if torch.equal(fused[0][1], base[0][1]) else f'rel L2 {rel_eps:.2e}'}; head fusion on under pins: "
          f"{head_runs[0]} dec1.conv2 ({head_runs[1]} with the head in the epilogue), {head_runs[2]} enc1.conv2 ({head_runs[3]} "
          f"storing the pool alone)")
    print("  strip tiles run, by picture width: " + "; ".join(
        f"{w} px {_hip.KIND_NAMES[k]} " + " ".join(f"{bm}x{bn}" for bm, bn in sorted(t)) for (w, k), t in sorted(strip_ran.items())))
    assert not failures, f"{c.name}: {len(failures)} failures:\n  " + "\n  ".join(failures[:40])
    # the one choice the rules admit and the launcher refuses: stripk's 64 x 64 tile (one strip item per thread) on picture
    # rows of more than 31 pixels
    for j, slot, bm, bn, _, kind in refused:
        assert (kind & 7, bm, bn) == (5, 64, 64) and level(c, j)[1] > 31, f"{c.name}: launch {(j, slot, bm, bn, kind)} refused"
    for (j, slot), kinds in admitted.items():
        assert seen[(j, slot)] == kinds, f"{c.name}: {engine.BLOCK_NAMES[j]}.{SLOT_NAMES[slot]} ran kinds {sorted(seen[(j, slot)])} of {sorted(kinds)}"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_conv_launches_block_by_block_vs_float64(case, models, cpu_threads, stats):
    run_case(case, models, stats)


# ------------------------------------------------------------------ the 2x2 max pool a pinned conv2 launch leaves behind
POOL_SHAPES = (
    Case("P_sf0.5_16x16_B5", 0.5, 16, 16, 5, 2, 0, 1, 0, 21),    # 16 / 8 px: the tile epilogues pool; splits: the slab sum pools
    Case("P_sf0.5_16x48_B3", 0.5, 16, 48, 3, 2, 0, 1, 0, 22),    # 48 .. 6 px: maxpool_kernel, and the slab sum under splits
    Case("P_sf0.3_32x32_B3", 0.3, 32, 32, 3, 2, 0, 1, 0, 23),    # 38 / 76 channels; 32 px: maxpool_kernel; then 16 .. 4 px
)
POOL_PATHS = ("tile epilogue", "slab sum", "maxpool_kernel")


def pool_path(c, j, splits):
    """which launch writes enc(j+1)'s pooled output (resolve_forward's pool_fused, heights and widths being even): the slab
    sum of a split conv2, else conv2's staged epilogue where W is a power of two <= 16, else maxpool_kernel"""
    w = level(c, j)[1]
    return POOL_PATHS[1] if splits > 1 else POOL_PATHS[0] if w <= 16 and w & (w - 1) == 0 else POOL_PATHS[2]


def pool_reference(a):
    """2x2 max pool of an NHWC block output, by torch on the device (exact: a maximum rounds nothing)"""
    return F.max_pool2d(a.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)


@pytest.mark.parametrize("case", POOL_SHAPES, ids=[c.name for c in POOL_SHAPES])
def test_pinned_conv2_launches_write_the_max_pool(case, models):
    """For j = enc1 .. enc4 every admissible conv2 pin (each tile, kind, split count, with and without the folded skip), with
    block j + 1 transparent: block j + 1's output then IS the pooled tensor the pinned launch (or maxpool_kernel behind it)
    wrote, and must equal max_pool2d of block j's output of the same run, number for number, under both poisons.  (The 0 / 1
    selection of transparent enc2 is exact in the split-bf16 walk too: the three bf16 planes of x sum to x, the other
    products are 0.)  Which of the three pool paths a pin takes follows from the rule and the reported split count; every path
    the shape's levels allow must have run."""
    c = case
    sd32 = {k: v.float() for k, v in models(c.sf).state_dict().items() if v.dtype.is_floating_point}
    found, failures, pins, refused, paths = None, [], 0, [], defaultdict(int)
    for j in range(4):
        run = Runner(c, transparent(sd32, j + 1))
        run.h.ensure_plan(run.rows, c.H, c.W, c.B, c.single, tune=False)
        if found is None:
            found = run.admissible(range(4), [2])       # (the rules see shapes, not weights: one enumeration serves all four)
        cout, cnext = run.couts[j], run.couts[j + 1]
        sel = torch.arange(cnext, device=DEV) % cout
        for key in sorted(k for k in found if k[0] == j):
            what = f"{engine.BLOCK_NAMES[j]}.conv2 {_hip.KIND_NAMES[key[5] & 7]} {key[2]}x{key[3]} s{key[4]}{' +skip' if key[5] & 8 else ''}"
            assert run.pin(j, 2, *found[key]), what
            assert run.report(j, 2)[:4] == key[2:], f"{what}: resolves differently on this handle"
            path = pool_path(c, j, key[4])
            got, why, status = [], [], 0
            for value in POISONS:
                status = run.poisoned_forward(value)
                if status < 0:
                    break
                check(status, f"dt_unet_forward ({what})")
                nxt = run.act(j + 1)
                if not torch.equal(nxt[..., :cnext], pool_reference(run.act(j)[..., :cout])[..., sel]):
                    why.append(f"poison {value}: block {j + 1}'s input is not the 2x2 max pool of block {j}'s output")
                if (nxt[..., cnext:] != 0).any().item():
                    why.append(f"poison {value}: nonzero padding channels")
                got.append(nxt.clone())
            if status < 0:
                refused.append(key)
                continue
            if not torch.equal(bits(got[0]), bits(got[1])):
                why.append("the pooled tensor differs between the poisons")
            pins += 1
            paths[path] += 1
            if why:
                failures.append(f"{what} (pool by {path}): " + "; ".join(why))
    print(f"\n{c.name}: {pins} conv2 pins, pool written by: " + ", ".join(f"{p} {paths[p]}" for p in POOL_PATHS) + f"; refused at launch: {refused}")
    assert not failures, f"{c.name}: {len(failures)} of {pins} pins fail:\n  " + "\n  ".join(failures[:40])
    for j, slot, bm, bn, _, kind in refused:
        assert (kind & 7, bm, bn) == (5, 64, 64) and level(c, j)[1] > 31, f"{c.name}: launch {(j, slot, bm, bn, kind)} refused"
    # enc2 .. enc4 are splittable at these sizes (fewer than 32768 GEMM rows), enc1 never is
    allowed = {POOL_PATHS[1]} | {pool_path(c, j, 1) for j in range(4)}
    assert {p for p in POOL_PATHS if paths[p]} == allowed, f"{c.name}: pool paths run {dict(paths)}, the rule allows {sorted(allowed)}"


# ------------------------------------------------------------------ more than two condition rows per image
@pytest.mark.parametrize("sf,shared", [(0.1, True), (0.2, True), (0.5, True), (0.5, False)],
                         ids=["sf0.1-fused", "sf0.2-fused", "sf0.5-shared-enc1", "sf0.5-per-pass-enc1"])
@pytest.mark.parametrize("n_pass", [3, 4])
def test_forward_with_three_and_four_passes(models, monkeypatch, sf, shared, n_pass):
    """dt_unet_forward accepts any n_pass (e.g. cond rows NONE / ZERO / ONE): the fused small-model kernel, enc1 shared by
    all passes (n_dup = n_pass) and one enc1 per pass, every row against the oracle"""
    if not shared:
        monkeypatch.setenv("DT_NO_SHARED_ENC1", "1")     # read by dt_unet_create
    sd = {k: v.float() for k, v in models(sf).state_dict().items()}
    h = engine.UNetHandle(sd, DEV)
    monkeypatch.delenv("DT_NO_SHARED_ENC1", raising=False)
    assert h.fused_active(16, 16) == (sf < 0.3) and h._shared_enc1 == shared
    B = 5
    x = torch.randn(B, 3, 16, 16, generator=torch.Generator().manual_seed(40 + n_pass))
    ts = [3, 17, 29, 40][:n_pass]
    modes = [COND_NONE, COND_ZERO, COND_ONE, COND_ONE][:n_pass]
    got = h.forward(x.to(DEV), h.time_bias(ts, modes), n_pass, B).cpu().numpy()
    assert got.shape == (n_pass * B, 3, 16, 16)
    for p, (t, m) in enumerate(zip(ts, modes)):
        cond = None if m == COND_NONE else torch.full((B, 1), 0.0 if m == COND_ZERO else 1.0)
        with torch.no_grad():
            want = unet_ref.unet_forward(sd, x, torch.full((B,), t), cond).numpy()
        err = np.abs(got[p * B:(p + 1) * B] - want)
        tol = 2e-5 + 1e-4 * np.abs(want)
        assert np.all(err <= tol), f"sf {sf} n_pass {n_pass} pass {p}: max err {err.max():.3e}"
