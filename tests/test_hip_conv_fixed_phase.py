"""The row arithmetic around the convolution kernels' tap loop (csrc/dt_conv_rows.h), on the device, in the shapes where a
division replaced by a multiply-shift pair could go wrong: block by block against float64, through the entry and with the
tolerances of tests/test_hip_conv_blocks.py (pinned launch, dt_unet_debug_activation, TAU * S elementwise, per-image
relative L2 and RMS, zero padding, NaN / 1e30 poisoning).

  * conv1 with one time-bias row per sample (m_per_tb = H * W) on 4 x 4 and 2 x 2 pictures, 70 batch rows: a tile holds 4 to
    64 time-bias rows and the last tile is partial; models with 12 -> 16 padded channels (sf 0.2) and with the 64 -> 128
    channel block (sf 1.0);
  * two and three passes of 3 images at 4 x 4: m_per_tb = 48, so the pass boundary falls inside every tile;
  * the dual-output enc1.conv2 at 16 x 16 with dup_skip = 256 (one single-pass image in front of two CFG images) and with
    dup_skip = 0, for images of 1, 2 and 3 channels (the picture-skip recomputed from the NCHW image);
  * a pooled conv2 output on a 6 x 6 picture (48 x 48 images, enc4), unsplit and through splitk_epilogue_kernel, and split
    conv1 launches (no pool) on the same level, read back exactly through a transparent next block.

Every kind runs in each group, the exact-fp32 GEMM (what DT_PRECISION=fp32 launches) among them.  enc1.conv2 on 8 x 8
pictures is not reachable through the forward (five levels need 16 pixels); its arithmetic at 8 x 8 is in
tests/test_conv_row_math.py."""
import pytest
import torch

import test_hip_conv_blocks as blocks
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd._hip import COND_NONE, COND_ONE, COND_ZERO, check
from fused_readout import transparent
from test_hip_conv_blocks import Case, Runner, bits, cpu_threads  # noqa: F401  (cpu_threads: the float64 references' thread limit)

pytestmark = pytest.mark.gpu
DEV = blocks.DEV

# (bm, bn, splits, kind, fuse) requests; the rules resolve each to a form the layer admits (or refuse it), duplicates drop out
TILES = [(64, 64), (128, 64), (256, 64), (64, 128), (128, 128)]
UNSPLIT = [(bm, bn, 1, kind, 0) for kind in (0, 1, 3, 4, 5) for bm, bn in TILES]
SPLIT = [(64, 64, s, kind, 0) for kind in (0, 1) for s in (3, 9)] + [(bm, 64, s, kind, 0) for kind in (3, 4, 5) for s in (2, 4) for bm in (64, 128)]


def state(model):
    return {k: v.float() for k, v in model.state_dict().items() if v.dtype.is_floating_point}


class ImageRunner(Runner):
    """Runner on images of `ch` channels"""

    def __init__(self, c, sd32, ch):
        super().__init__(c, sd32)
        g = torch.Generator().manual_seed(2000 + c.seed)
        self.x = torch.randn(c.B, ch, c.H, c.W, generator=g)
        self.x_dev = self.x.to(DEV)
        self.eps = torch.empty(self.rows, ch, c.H, c.W, dtype=torch.float32, device=DEV)


def references(run, sd32):
    """the heuristic plan's block outputs (under both poisons) and every block's float64 reference and bound from them"""
    c = run.c
    run.h.ensure_plan(run.rows, c.H, c.W, c.B, c.single, tune=False)
    run.h.set_precision(_hip.PREC_AUTO)
    base = []
    for value in blocks.POISONS:
        check(run.poisoned_forward(value), "dt_unet_forward")
        base.append([run.act(j).clone() for j in range(8)])
    for j in range(8):
        assert torch.equal(bits(base[0][j]), bits(base[1][j])), f"{c.name}: heuristic plan, block {j} reads unwritten memory"
    sd64 = {k: v.double() for k, v in sd32.items()}
    acts = [a[..., :cout].permute(0, 3, 1, 2).double().cpu() for a, cout in zip(base[0], run.couts)]
    temb = blocks.row_temb(sd32, run.conds, c.tb_div)
    refs = blocks.block_references(sd64, run.x.double()[run.imgs], acts, temb)
    return base[0], {j: (r.to(DEV), s.to(DEV)) for j, (r, s) in refs.items()}


def check_pins(run, base, refs, targets, requests, need_kinds):
    """every distinct launch the requests resolve to on the target (block, slot)s, against the block's float64 reference"""
    c, failures, seen = run.c, [], {}
    for j, slot in targets:
        for req in requests:
            if not run.pin(j, slot, *req):
                continue
            rep = run.report(j, slot)
            if rep[0] == 0 or (j, slot) + rep[:4] in seen:
                continue
            what = f"{c.name} {engine.BLOCK_NAMES[j]}.{blocks.SLOT_NAMES[slot]} {_hip.KIND_NAMES[rep[3] & 7]} {rep[0]}x{rep[1]} s{rep[2]}"
            outs, status = [], 0
            for value in blocks.POISONS:
                status = run.poisoned_forward(value)
                if status < 0:
                    break
                check(status, what)
                outs.append(run.act(j).clone())
                if any((bits(run.act(u)) != bits(base[u])).any().item() for u in range(j)):
                    failures.append(f"{what}: a block upstream of the pinned one changed")
            if status < 0:
                continue                               # (refused at the launch: its LDS or reach)
            seen[(j, slot) + rep[:4]] = rep[3] & 7
            ref, S = refs[j]
            bad, ratio, rel, pad, rms = blocks.check_block(outs[0], ref, S, run.couts[j]).tolist()
            print(f"{what}: max err/S {ratio * 2 ** 24:.3f} * 2^-24, rel L2 {rel:.2e}, RMS err/S {rms * 2 ** 24:.4f} * 2^-24")
            if not torch.equal(bits(outs[0]), bits(outs[1])):
                failures.append(f"{what}: block output differs between NaN- and 1e30-poisoned workspaces")
            if bad:
                failures.append(f"{what}: |err| > {blocks.C_TAU} * 2^-24 * S (max err/S = {ratio * 2 ** 24:.2f} * 2^-24)")
            if rel > blocks.REL_L2:
                failures.append(f"{what}: per-image relative L2 error {rel:.3e} > {blocks.REL_L2:.0e}")
            if rms * 2 ** 24 > blocks.RMS_C:
                failures.append(f"{what}: per-image RMS of err/S {rms * 2 ** 24:.3f} * 2^-24 > {blocks.RMS_C} * 2^-24")
            if pad:
                failures.append(f"{what}: nonzero padding channels")
    run.h.set_precision(_hip.PREC_AUTO)
    assert not failures, f"{len(failures)} failures:\n  " + "\n  ".join(failures[:40])
    for target in targets:
        kinds = {k for key, k in seen.items() if key[:2] == target}
        assert need_kinds <= kinds, f"{c.name}: {target} ran kinds {sorted(kinds)}, not all of {sorted(need_kinds)}"
    return seen


@pytest.mark.parametrize("sf", [0.2, 1.0], ids=["12_to_16_channels", "64_to_128_channels"])
def test_conv1_with_a_time_bias_row_per_sample(models, cpu_threads, sf):
    """m_per_tb = H * W: 16 rows per time-bias row at 4 x 4 (enc3, dec3), 4 at 2 x 2 (enc4, dec4), 64 at 8 x 8 (enc2, the
    64 -> 128 channel block at sf 1.0); 70 batch rows leave 1120 = 4 * 256 + 96 and 280 = 256 + 24 GEMM rows"""
    c = Case(f"tb_row_per_sample_sf{sf}", sf, 16, 16, 35, 2, 0, 1, 0, 31)
    sd32 = state(models(sf))
    run = Runner(c, sd32)
    assert len(run.conds) == 70
    base, refs = references(run, sd32)
    seen = check_pins(run, base, refs, [(1, 1), (2, 1), (3, 1), (5, 1), (6, 1)], UNSPLIT + SPLIT, {0, 1, 3, 4, 5})
    assert any(key[4] > 1 for key in seen), "no split conv1 launch (splitk_epilogue_kernel adds the time bias there)"


@pytest.mark.parametrize("n_pass", [2, 3])
def test_pass_boundary_inside_a_tile(models, cpu_threads, n_pass):
    """3 images, one time-bias row per pass: m_per_tb = 48 at 4 x 4 and 12 at 2 x 2, no multiple or divisor of a tile height"""
    c = Case(f"pass_boundary_{n_pass}_passes", 0.5, 16, 16, 3, n_pass, 0, 3, 0, 32 + n_pass)
    sd32 = state(models(0.5))
    run = Runner(c, sd32)
    run.conds = [(9, COND_NONE), (9, COND_ONE), (510, COND_ZERO)][:n_pass]
    run.tb = run.h.time_bias([t for t, _ in run.conds], [m for _, m in run.conds])
    base, refs = references(run, sd32)
    check_pins(run, base, refs, [(2, 1), (3, 1), (6, 1), (0, 2)], UNSPLIT + SPLIT, {0, 1})


@pytest.mark.parametrize("single", [1, 0], ids=["dup_skip_256", "dup_skip_0"])
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_dual_output_enc1_conv2(cpu_threads, ch, single):
    """enc1.conv2 once for both passes: per pass the class-bias row of the unit's time-bias row (one per batch row here), the
    image skip from the `ch`-channel NCHW image, pass 1 of image b >= single at row dup_rows + m - dup_skip"""
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model
    cfg = Config()
    cfg.image_size, cfg.channels = 16, ch
    sd32 = state(make_model(DiffusionUNet, cfg, 0.5))
    c = Case(f"dual_ch{ch}_single{single}", 0.5, 16, 16, 2 + single, 2, single, 1, 0, 40 + ch)
    run = ImageRunner(c, sd32, ch)
    base, refs = references(run, sd32)
    fused = [r[:4] + (1,) for r in UNSPLIT if r[3] != 0]
    seen = check_pins(run, base, refs, [(0, 2)], UNSPLIT + fused, {0, 1, 3, 4, 5})
    # with head fusion on (the default) the same pins store the pool alone: enc2's output must not change
    run.h.set_head_fusion(True)
    for key in sorted(seen):
        assert run.pin(0, 2, key[2], key[3], key[4], key[5] & 7, key[5] >> 3)
        run.h.set_head_fusion(False)
        check(run.poisoned_forward(float("nan")), "head fusion off")
        off = run.act(1).clone()
        run.h.set_head_fusion(True)
        check(run.poisoned_forward(float("nan")), "head fusion on")
        assert torch.equal(bits(run.act(1)), bits(off)), f"{c.name} {key}: the pooled output under skip_out changes enc2"
    run.h.set_head_fusion(False)


def test_pool_and_split_k_on_6x6_pictures(models):
    """48 x 48 images: enc4 works on 6 x 6 pictures.  Its conv2 pins, unsplit (maxpool_kernel pools) and split (the slab sum of
    splitk_epilogue_kernel pools), with the bottleneck transparent: its output then is the pooled tensor, number for number.
    Split conv1 pins of the same block (slab sum without a pool, with the time bias) against float64."""
    c = Case("pool_6x6", 0.5, 48, 48, 3, 2, 0, 1, 0, 51)
    sd32 = state(models(0.5))
    j = 3
    run = Runner(c, transparent(sd32, j + 1))
    run.h.ensure_plan(run.rows, c.H, c.W, c.B, c.single, tune=False)
    cout, cnext = run.couts[j], run.couts[j + 1]
    sel = torch.arange(cnext, device=DEV) % cout
    splits_seen, failures, done = set(), [], set()
    for req in UNSPLIT + SPLIT + [(64, 64, 8, 3, 0), (64, 64, 8, 5, 0)]:
        if not run.pin(j, 2, *req):
            continue
        rep = run.report(j, 2)
        if rep[:4] in done:
            continue
        got = []
        for value in blocks.POISONS:
            status = run.poisoned_forward(value)
            if status < 0:
                break
            check(status, f"pool pin {rep}")
            nxt = run.act(j + 1)
            if not torch.equal(nxt[..., :cnext], blocks.pool_reference(run.act(j)[..., :cout])[..., sel]):
                failures.append(f"conv2 {rep}, poison {value}: the bottleneck's input is not the 2x2 max pool of enc4's output")
            got.append(nxt.clone())
        if len(got) == 2:
            done.add(rep[:4])
            splits_seen.add(rep[2] > 1)
            if not torch.equal(bits(got[0]), bits(got[1])):
                failures.append(f"conv2 {rep}: the pooled tensor differs between the poisons")
    assert not failures, "\n  ".join(failures[:40])
    assert splits_seen == {False, True}, f"pool paths run: split {splits_seen}"

    run = Runner(c, sd32)
    base, refs = references(run, sd32)
    seen = check_pins(run, base, refs, [(j, 1)], SPLIT + [(64, 64, 1, 1, 0)], {0, 1})
    assert any(key[4] > 1 for key in seen), "no split conv1 launch"
