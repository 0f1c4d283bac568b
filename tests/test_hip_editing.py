"""GPU: the editing stage (include/dt_hip_edit.h, distillation_trajectories_amd/editing/).

  1. one masked step (dt_cfg_update_masked) against the torch-CPU expression, bit for bit
  2. the start state (dt_edit_start) against torch CPU, bit for bit
  3. the masked loop on the fused and on the layered path: the known region is kept exactly, a mask of ones is the unmasked
     loop, a row's bits do not depend on its batch; loops of 1 and of 70 steps, one channel, 32 x 32, CFG and mixed batches;
     fused against layered within tests/test_hip_fused.py's bound for that comparison (2e-5 of the largest magnitude)
  4. the hole statistics (dt_masked_pair_stats) against numpy float64: relative error <= 1e-12 (at most 3072 terms, each
     rounded to 2^-53: at most 3.5e-13), repeat calls bit-identical
  5. the three mirrored modules against the reference's own trajectories and images (tests/golden/reference_vectors_editing.*)
     within the project's trajectory tolerance (rtol 1e-4, atol 1e-4: tests/test_hip_parity.py)
  6. the sweeps: every cell equals the same cell run alone, bit for bit
"""
import numpy as np
import pytest
import torch

import editing_ref as er
from distillation_trajectories_amd import engine
from distillation_trajectories_amd._hip import COND_NONE, COND_ONE, COND_ZERO, RULE_ENGINE, RULE_MANAGER, RULE_PSAMPLE
from distillation_trajectories_amd.config import Config
from distillation_trajectories_amd.editing import (inpainting_sweep, latent_manipulation, manipulation_sweep, masked_inpainting,
                                                   prompt_editing)
from distillation_trajectories_amd.models import DiffusionUNet
from distillation_trajectories_amd.synthetic import make_model, state_dict_digest
from distillation_trajectories_amd.utils.diffusion import get_diffusion_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = lambda v: torch.tensor(v, dtype=torch.float32)   # noqa: E731


def config(T=8, size=16, channels=3):
    cfg = Config()
    cfg.image_size, cfg.channels, cfg.timesteps = size, channels, T
    return cfg


_MODELS = {}


def model(sf, channels=3):
    """one device model per (size factor, channels) for the whole module"""
    key = (sf, channels)
    if key not in _MODELS:
        _MODELS[key] = make_model(DiffusionUNet, config(channels=channels), sf).to(DEV)
    return _MODELS[key]


def handle(sf, fused, channels=3):
    h = engine.UNetHandle.for_module(model(sf, channels))
    h.set_fused(fused)
    return h


def rect(E, C, lo, hi, value=1.0):
    """[E] mask of a C-channel square picture: `value` on rows / columns lo .. hi-1, zero elsewhere"""
    side = int(round((E // C) ** 0.5))
    m = torch.zeros(C, side, side)
    m[:, lo:hi, lo:hi] = value
    return m.reshape(-1)


def i32(v):
    return torch.tensor(v, dtype=torch.int32).to(DEV)


# ---------------------------------------------------------------------- 1. one masked step
def _step_cpu(rule, x, eu, ec, z, coef, noise, w):
    c0, c1, c2 = (f32(v) for v in coef)
    eps = eu if ec is None else eu + w * (ec - eu)
    if rule == RULE_ENGINE:
        return (c0 * x - c1 * eps) + c2 * z if noise else None
    zz = z if noise else torch.zeros_like(x)
    if rule == RULE_PSAMPLE:
        return c0 * (x - c1 * eps) + zz * c2
    return (x - c0 * eps) / c1 + c2 * zz


@pytest.mark.parametrize("rule", [RULE_ENGINE, RULE_PSAMPLE, RULE_MANAGER])
@pytest.mark.parametrize("E", [4, 768])
def test_masked_step_is_the_torch_cpu_expression(rule, E):
    B = 3
    g = torch.Generator().manual_seed(100 * rule + E)
    x, eu, ec = (torch.randn(B, E, generator=g) for _ in range(3))
    z = torch.randn(B + 2, E, generator=g)
    z_row = torch.tensor([2, 0, 4])
    known = torch.rand(4, E, generator=g) * 2 - 1
    binary = (torch.rand(4, E, generator=g) < 0.5).float()
    soft = torch.tensor([0.0, 0.25, 1.0, 0.6])[torch.randint(0, 4, (4, E), generator=g)]
    w_rows = torch.tensor([0.0, 3.0, 7.5])
    coef = {RULE_ENGINE: (1.0123, 0.0456, 0.0789), RULE_PSAMPLE: (1.02, 0.07, 0.05), RULE_MANAGER: (0.1, 0.95, 0.02)}[rule]
    dev = lambda t: None if t is None else t.to(DEV)   # noqa: E731
    for mask in (binary, soft):
        for cfg in (False, True):
            for noise in (0, 1):
                for rows in (None, (torch.tensor([3, 1, 1]), torch.tensor([0, 2, 0]))):
                    mr, kr = rows if rows else (torch.arange(B), torch.arange(B))
                    w = w_rows.reshape(B, 1) if cfg else None
                    xn = _step_cpu(rule, x, eu, ec if cfg else None, z[z_row], coef, noise, w)
                    want = x if xn is None else mask[mr] * xn + (1 - mask[mr]) * known[kr]       # (ENGINE, t == 0: x unblended)
                    got = engine.cfg_update_masked(rule, dev(x), dev(eu), dev(ec) if cfg else None, dev(z), coef, noise, dev(mask),
                                                   dev(known), None if rows is None else i32(mr.tolist()),
                                                   None if rows is None else i32(kr.tolist()), w=dev(w_rows) if cfg else None,
                                                   z_row=i32(z_row.tolist()))
                    assert torch.equal(got.cpu(), want), (rule, E, cfg, noise, rows is not None)
    # a mask of ones is dt_cfg_update
    ones = torch.ones(B, E)
    for noise in (0, 1):
        a = engine.cfg_update_masked(rule, dev(x), dev(eu), dev(ec), dev(z), coef, noise, dev(ones), dev(known), w=dev(w_rows))
        b = engine.cfg_update(rule, dev(x), dev(eu), dev(ec), dev(z), coef, noise, w=dev(w_rows))
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


# ---------------------------------------------------------------------- 2. the start state
@pytest.mark.parametrize("E", [256, 768])
def test_edit_start_is_the_torch_cpu_expression(E):
    B = 5
    g = torch.Generator().manual_seed(E)
    img = torch.rand(2, E, generator=g)
    z = torch.randn(3, E, generator=g)
    mask = torch.stack([rect(E, E // 256, 4, 11), torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (E,), generator=g)]])
    ir, zr, mr = torch.tensor([0, 1, 1, 0, 1]), torch.tensor([2, 2, 0, 1, 0]), torch.tensor([1, 0, 0, 1, 1])
    known, x = engine.edit_start(img.to(DEV), z.to(DEV), mask.to(DEV), B, i32(ir.tolist()), i32(zr.tolist()), i32(mr.tolist()))
    want_known = 2 * img - 1
    assert torch.equal(known.cpu(), want_known)
    assert torch.equal(x.cpu(), mask[mr] * z[zr] + (1 - mask[mr]) * want_known[ir])
    # without row tables: cell b reads row b of everything
    known, x = engine.edit_start(img.to(DEV), z.to(DEV), mask.to(DEV), 2)
    assert torch.equal(x.cpu(), mask * z[:2] + (1 - mask) * want_known)


# ---------------------------------------------------------------------- 3. the masked loop
def loop_inputs(B, n_steps, E, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, E, generator=g), torch.randn(n_steps * B + 3, E, generator=g), torch.rand(3, E, generator=g) * 2 - 1)


def schedule(n_steps):
    """(timesteps, coefficients, has_noise) of an ENGINE loop that ends with the dead t = 0 step"""
    ts = [t % 50 for t in range(n_steps - 1, -1, -1)]
    coef = [(0.98 + 0.0002 * (i % 40), 0.05 + 0.001 * (i % 40), 0.01 * (1 + i % 5)) for i in range(n_steps)]
    return ts, coef, [i < n_steps - 1 for i in range(n_steps)]


def run_loop(h, x0, z, n_steps, size=16, mask=None, known=None, mask_row=None, known_row=None, z_row=None, rule=RULE_ENGINE):
    B, E = x0.shape
    ts, coef, noise = schedule(n_steps)
    if rule != RULE_ENGINE:
        coef, noise = [(1.01, 0.03, 0.02) if rule == RULE_PSAMPLE else (0.1, 0.95, 0.02)] * n_steps, [True] * n_steps
    tb = h.time_bias(ts, [COND_NONE] * n_steps)
    traj = torch.empty(n_steps + 1, B, E, device=DEV)
    traj[0] = x0.to(DEV)
    kw = dict(z=z.to(DEV), z_row=z_row, z_shift=[i * 2 for i in range(n_steps)])
    if mask is None:
        h.sample(rule, traj, size, size, tb, 1, coef, noise, **kw)
    else:
        h.sample_masked(rule, traj, size, size, tb, 1, coef, noise, mask.to(DEV), known.to(DEV), mask_row, known_row, **kw)
    return traj.cpu()


PATHS = [(0.1, True), (0.2, True), (0.1, False), (0.2, False), (0.5, False)]


@pytest.mark.parametrize("sf,fused", PATHS)
def test_masked_loop_keeps_the_known_region_and_rows_do_not_depend_on_the_batch(sf, fused):
    h = handle(sf, fused)
    assert h.fused_active(16, 16) == fused
    B, n, E = 5, 8, 768
    x0, z, known = loop_inputs(B, n, E, 11)
    masks = torch.stack([rect(E, 3, 4, 11), 1 - rect(E, 3, 2, 9)])
    mr, kr, zr = [0, 1, 1, 0, 1], [2, 0, 1, 1, 2], [3, 0, 4, 1, 2]
    x0 = masks[mr] * x0 + (1 - masks[mr]) * known[kr]
    full = run_loop(h, x0, z, n, mask=masks, known=known, mask_row=i32(mr), known_row=i32(kr), z_row=i32(zr))
    assert torch.isfinite(full).all()
    for b in range(B):                                       # every slot keeps the known image where the mask is 0
        hole = masks[mr[b]] == 0
        assert 0 < hole.sum() < E
        assert np.array_equal(full[:, b, hole].numpy(), known[kr[b]][hole].expand(n + 1, -1).numpy()), b
        assert not torch.equal(full[1, b, ~hole], full[0, b, ~hole])
    assert torch.equal(full[-1], full[-2])                   # t == 0: recorded unchanged
    # B = 1, 3 (one more than a full group of two), 4; shared tables (rows materialised, no row table) or per-row tables
    for rows in ([3], [0, 1, 4], [4, 2, 1, 0]):
        sub = run_loop(h, x0[rows], z, n, mask=masks, known=known, mask_row=i32([mr[b] for b in rows]),
                       known_row=i32([kr[b] for b in rows]), z_row=i32([zr[b] for b in rows]))
        assert np.array_equal(sub.numpy(), full[:, rows].numpy()), rows
        flat = run_loop(h, x0[rows], z, n, mask=masks[[mr[b] for b in rows]], known=known[[kr[b] for b in rows]],
                        z_row=i32([zr[b] for b in rows]))
        assert np.array_equal(flat.numpy(), sub.numpy()), rows
    again = run_loop(h, x0, z, n, mask=masks, known=known, mask_row=i32(mr), known_row=i32(kr), z_row=i32(zr))
    assert torch.equal(again, full)


@pytest.mark.parametrize("sf,fused", PATHS)
@pytest.mark.parametrize("rule", [RULE_ENGINE, RULE_PSAMPLE, RULE_MANAGER])
def test_mask_of_ones_is_the_unmasked_loop(sf, fused, rule):
    h = handle(sf, fused)
    B, n, E = 3, 8, 768
    x0, z, known = loop_inputs(B, n, E, 12 + rule)
    plain = run_loop(h, x0, z, n, rule=rule)
    masked = run_loop(h, x0, z, n, mask=torch.ones(1, E), known=known, mask_row=i32([0] * B), known_row=i32([2, 1, 0]), rule=rule)
    assert np.array_equal(masked.numpy(), plain.numpy())


@pytest.mark.parametrize("sf,fused", PATHS)
def test_first_masked_loop_step_is_forward_plus_masked_update(sf, fused):
    """a soft mask through the loop against forward + dt_cfg_update_masked (test 1 pins that step to torch CPU): the blend's
    arithmetic is shared (dt_update_math.h), so equal predictions give equal bits"""
    h = handle(sf, fused)
    B, E = 3, 768
    x0, z, known = loop_inputs(B, 1, E, 40)
    soft = torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (2, E), generator=torch.Generator().manual_seed(4))]
    mr = i32([1, 0, 1])
    tb = h.time_bias([30], [COND_NONE])
    coef = (1.02, 0.07, 0.05)
    for rule in (RULE_ENGINE, RULE_PSAMPLE, RULE_MANAGER):
        traj = torch.empty(2, B, E, device=DEV)
        traj[0] = x0.to(DEV)
        h.sample_masked(rule, traj, 16, 16, tb, 1, [coef], [True], soft.to(DEV), known.to(DEV), mr, None, z=z.to(DEV))
        eps = h.forward(x0.reshape(B, 3, 16, 16).to(DEV), tb, 1, B).reshape(B, E)
        want = engine.cfg_update_masked(rule, x0.to(DEV), eps, None, z.to(DEV), coef, True, soft.to(DEV), known.to(DEV), mr)
        assert torch.equal(traj[1], want), rule


_SEVENTY = {}      # (fused, steps) -> trajectory of the test below, compared across the paths by the test after it


@pytest.mark.parametrize("sf,fused", [(0.1, True), (0.1, False)])
def test_masked_loops_of_one_and_of_seventy_steps(sf, fused):
    h = handle(sf, fused)
    B, E = 3, 768
    masks = torch.stack([rect(E, 3, 3, 12)])
    for n in (1, 70):                                         # 70 > kFusedMaxSteps = 64: two fused launches, the mask travels
        x0, z, known = loop_inputs(B, n, E, n)
        x0 = masks[0] * x0 + (1 - masks[0]) * known
        ts, coef, noise = schedule(n)
        if n == 1:
            noise = [True]                                    # a single live step (t > 0)
        tb = h.time_bias(ts, [COND_NONE] * n)
        traj = torch.empty(n + 1, B, E, device=DEV)
        traj[0] = x0.to(DEV)
        h.sample_masked(RULE_ENGINE, traj, 16, 16, tb, 1, coef, noise, masks.to(DEV), known.to(DEV), i32([0] * B), None,
                        z=z.to(DEV), z_shift=[i * B for i in range(n)])
        got = traj.cpu()
        hole = masks[0] == 0
        assert torch.isfinite(got).all()
        assert np.array_equal(got[:, :, hole].numpy(), known[:, hole].expand(n + 1, -1, -1).numpy()), n
        assert not torch.equal(got[-1][:, ~hole], got[0][:, ~hole])
        _SEVENTY[(fused, n)] = got


def test_fused_and_layered_masked_loops_agree():
    """within the bound tests/test_hip_fused.py uses for the unmasked loops: 2e-5 of the largest magnitude"""
    if len(_SEVENTY) < 4:
        for sf, fused in [(0.1, True), (0.1, False)]:
            test_masked_loops_of_one_and_of_seventy_steps(sf, fused)
    for n in (1, 70):
        a, b = _SEVENTY[(True, n)], _SEVENTY[(False, n)]
        scale = b.abs().max().item()
        print(f"n = {n}: fused vs layered {(a - b).abs().max().item():.3e}, bound {2e-5 * scale:.3e}")
        assert (a - b).abs().max().item() <= 2e-5 * scale


def test_masked_loop_one_channel_and_32x32():
    for sf, fused, C, size in ((0.1, True, 1, 16), (0.1, False, 1, 16), (0.1, False, 3, 32)):
        h = handle(sf, fused, C)
        assert h.fused_active(size, size) == fused
        B, n, E = 3, 4, C * size * size
        x0, z, known = loop_inputs(B, n, E, 5 + C + size)
        mask = rect(E, C, 5, size - 3).reshape(1, E)
        x0 = mask * x0 + (1 - mask) * known
        got = run_loop(h, x0, z, n, size=size, mask=mask, known=known, mask_row=i32([0] * B))
        hole = mask[0] == 0
        assert torch.isfinite(got).all()
        assert np.array_equal(got[:, :, hole].numpy(), known[:, hole].expand(n + 1, -1, -1).numpy()), (C, size)
        ones = run_loop(h, x0, z, n, size=size, mask=torch.ones(1, E), known=known, mask_row=i32([0] * B))
        assert np.array_equal(ones.numpy(), run_loop(h, x0, z, n, size=size).numpy()), (C, size)
        one = run_loop(h, x0[1:2], z, n, size=size, mask=mask, known=known[1:2], z_row=i32([1]))
        assert np.array_equal(one[:, 0].numpy(), got[:, 1].numpy()), (C, size)


@pytest.mark.parametrize("sf,fused", [(0.2, True), (0.2, False), (0.5, False)])
def test_masked_cfg_and_mixed_batches(sf, fused):
    h = handle(sf, fused)
    n, E = 6, 768
    ts, coef, noise = schedule(n)
    mask = rect(E, 3, 4, 12).reshape(1, E)
    hole = mask[0] == 0
    # two-pass CFG batch, per-row guidance scales
    B = 3
    x0, z, known = loop_inputs(B, n, E, 21)
    x0 = mask * x0 + (1 - mask) * known
    tb = h.time_bias([t for t in ts for _ in (0, 1)], [COND_ZERO, COND_ONE] * n)
    w = torch.tensor([1.5, 3.0, 7.5]).to(DEV)
    kw = dict(z=z.to(DEV), z_shift=[i * B for i in range(n)], w=w)

    def cfg_run(m):
        traj = torch.empty(n + 1, B, E, device=DEV)
        traj[0] = x0.to(DEV)
        if m is None:
            h.sample(RULE_ENGINE, traj, 16, 16, tb, 2, coef, noise, **kw)
        else:
            h.sample_masked(RULE_ENGINE, traj, 16, 16, tb, 2, coef, noise, m.to(DEV), known.to(DEV), i32([0] * B), None, **kw)
        return traj.cpu()
    got = cfg_run(mask)
    assert np.array_equal(got[:, :, hole].numpy(), known[:, hole].expand(n + 1, -1, -1).numpy())
    assert np.array_equal(cfg_run(torch.ones(1, E)).numpy(), cfg_run(None).numpy())
    # mixed batch: S single-pass images, then two CFG blocks of S images
    S, G = 2, 2
    B = (1 + G) * S
    x0, z, known3 = loop_inputs(B, n, E, 22)
    known = known3[[0, 1, 2, 0, 1, 2]]
    x0 = mask * x0 + (1 - mask) * known
    tbm = h.time_bias([t for t in ts for _ in range(1 + 2 * G)], ([COND_NONE] + [COND_ZERO] * G + [COND_ONE] * G) * n)
    wm = torch.cat([torch.zeros(S), torch.tensor([3.0, 7.0]).repeat_interleave(S)]).to(DEV)
    zr = i32(list(range(S)) * (1 + G))

    def mixed_run(m):
        traj = torch.empty(n + 1, B, E, device=DEV)
        traj[0] = x0.to(DEV)
        if m is None:
            h.sample_mixed(RULE_ENGINE, traj, 16, 16, tbm, S, S, coef, noise, z.to(DEV), zr, [i * S for i in range(n)], wm)
        else:
            h.sample_masked(RULE_ENGINE, traj, 16, 16, tbm, 2, coef, noise, m.to(DEV), known.to(DEV), i32([0] * B), None,
                            z=z.to(DEV), z_row=zr, z_shift=[i * S for i in range(n)], w=wm, b_single=S, tb_div=S)
        return traj.cpu()
    got = mixed_run(mask)
    assert torch.isfinite(got).all()
    assert np.array_equal(got[:, :, hole].numpy(), known[:, hole].expand(n + 1, -1, -1).numpy())
    assert np.array_equal(mixed_run(torch.ones(1, E)).numpy(), mixed_run(None).numpy())


# ---------------------------------------------------------------------- 4. hole statistics
def _hole_ref(X, Y, m, k):
    X, Y, m, k = (np.asarray(a, dtype=np.float64) for a in (X, Y, m, k))
    d, dx, dy = X - Y, X - k, Y - k
    return np.stack([(m * d * d).sum(-1), (m * dx * dx).sum(-1), (m * dy * dy).sum(-1), ((1 - m) * d * d).sum(-1)], axis=-1)


@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("E", [4, 768, 3072])
def test_hole_statistics_against_numpy_float64(n, E):
    B = 3
    g = torch.Generator().manual_seed(n * 10000 + E)
    X, Y = torch.randn(n, B, E, generator=g), torch.randn(n, B, E, generator=g)
    known = torch.rand(2, E, generator=g) * 2 - 1
    mask = torch.stack([(torch.rand(E, generator=g) < 0.4).float(), torch.rand(E, generator=g)])
    mr, kr = [1, 0, 1], [0, 1, 1]
    got = engine.device_masked_pair_stats(X.to(DEV), Y.to(DEV), mask.to(DEV), known.to(DEV), i32(mr), i32(kr))
    want = _hole_ref(X.numpy(), Y.numpy(), mask[mr].numpy()[None], known[kr].numpy()[None]).transpose(1, 0, 2)   # [B, n, 4]
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, n, 4)
    g64, ok = got.cpu().numpy(), want > 0                       # (a sum of non-negative terms is 0 only if every term is)
    rel = np.abs(g64[ok] - want[ok]) / want[ok]
    print(f"n = {n}, E = {E}: worst relative error {rel.max():.3e}")
    assert rel.max() <= 1e-12 and (g64[~ok] == 0).all()
    again = engine.device_masked_pair_stats(X.to(DEV), Y.to(DEV), mask.to(DEV), known.to(DEV), i32(mr), i32(kr))
    assert torch.equal(again, got)
    flat = engine.device_masked_pair_stats(X.to(DEV), Y.to(DEV), mask[mr].to(DEV), known[kr].to(DEV))
    assert torch.equal(flat, got)


# ---------------------------------------------------------------------- 5. the mirrored modules against the reference's numbers
TOL = dict(rtol=1e-4, atol=1e-4)


def golden_model(sf):
    _, meta = er.golden()
    m = model(sf)
    assert state_dict_digest({k: v.cpu() for k, v in m.state_dict().items()}) == meta["state_dict_sha256"][str(sf)]
    handle(sf, sf < 0.3)
    return m


def params(T, augmented=True):
    dp = get_diffusion_params(T)
    if augmented:
        dp = dict(dp, timesteps=T, alphas=1 - dp["betas"])
    return dp


def check_traj(traj, arrays, key, timesteps):
    assert [t for _, t in traj] == timesteps and len(traj) == arrays[key].shape[0]
    for x, _ in traj:
        assert tuple(x.shape) == (1, 3, 16, 16) and x.device.type == "cuda"
    got = torch.stack([x for x, _ in traj]).cpu().numpy()
    print(f"{key}: max abs err {np.abs(got - arrays[key]).max():.3e}")
    assert np.allclose(got, arrays[key], **TOL), key


@pytest.mark.parametrize("name", ["inpaint_sf0.2", "inpaint_sf0.5", "inpaint_soft", "inpaint_none"])
def test_masked_inpainting_against_the_reference_vectors(name):
    arrays, meta = er.golden()
    case, T = meta["cases"][name], meta["T"]
    m = golden_model(case["sf"])
    image = None if name == "inpaint_none" else torch.from_numpy(arrays["image"].copy()).to(DEV)
    mask = {"inpaint_none": None, "inpaint_soft": torch.from_numpy(arrays["soft_mask_in"].copy()).to(DEV)}.get(name, arrays["rect_mask_in"])

    def call(dp):
        torch.manual_seed(meta["case_seed"])
        np.random.seed(meta["np_seed"])
        return masked_inpainting.apply_masked_inpainting(m, dp, image, mask, config(T), torch.device(DEV))
    res = call(params(T))
    assert sorted(res) == ["inpainted_image", "mask", "original_image", "trajectory"]
    assert res["mask"].dtype == torch.float32 and np.array_equal(res["mask"].cpu().numpy(), arrays[f"{name}/mask"])
    assert np.allclose(res["original_image"].cpu().numpy(), arrays[f"{name}/original"], **TOL)
    check_traj(res["trajectory"], arrays, f"{name}/trajectory", case["timesteps"])
    assert np.allclose(res["inpainted_image"].cpu().numpy(), arrays[f"{name}/inpainted"], **TOL)
    if name != "inpaint_soft":                               # binary masks: the known region of every state, exactly
        hole = res["mask"] == 0
        known = 2 * res["original_image"] - 1
        for x, _ in res["trajectory"]:
            assert torch.equal(x[hole], known[hole])
    # the plain dict of get_diffusion_params (no "timesteps", no "alphas") gives the same result
    plain = call(params(T, augmented=False))
    assert torch.equal(plain["inpainted_image"], res["inpainted_image"])
    assert all(torch.equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(plain["trajectory"], res["trajectory"]))
    assert "trajectory" not in masked_inpainting.apply_masked_inpainting(m, params(T), res["original_image"], res["mask"][0, 0],
                                                                         config(T), torch.device(DEV), record_trajectory=False)


def test_latent_manipulation_against_the_reference_vectors():
    arrays, meta = er.golden()
    case, T = meta["cases"]["manip"], meta["T"]
    m = golden_model(0.2)
    torch.manual_seed(meta["case_seed"])
    res = latent_manipulation.apply_latent_manipulation(m, params(T), "random", case["strength"], config(T), torch.device(DEV),
                                                        num_samples=2)
    assert sorted(res) == ["direction", "manipulated_images", "original_images", "strength", "trajectories"]
    assert np.array_equal(res["direction"].cpu().numpy(), arrays["manip/direction"]) and res["strength"] == case["strength"]
    assert len(res["original_images"]) == len(res["manipulated_images"]) == len(res["trajectories"]) == 2
    for i in range(2):
        for kind in ("original", "manipulated"):
            check_traj(res["trajectories"][i][kind], arrays, f"manip/{kind}_trajectory_{i}", case["timesteps"][f"{kind}_{i}"])
            assert np.allclose(res[f"{kind}_images"][i].cpu().numpy(), arrays[f"manip/{kind}_image_{i}"], **TOL)
    torch.manual_seed(meta["case_seed"])
    plain = latent_manipulation.apply_latent_manipulation(m, params(T, False), "random", case["strength"], config(T),
                                                          torch.device(DEV), num_samples=2)
    assert all(torch.equal(a, b) for a, b in zip(plain["manipulated_images"], res["manipulated_images"]))
    # latent + strength * direction and the image map: the torch ops on the device give torch CPU's bits
    latent, direction = res["trajectories"][0]["original"][-1][0], res["direction"]
    dev = latent + 2.0 * direction.reshape(latent.shape)
    cpu = latent.cpu() + 2.0 * direction.cpu().reshape(latent.shape)
    assert torch.equal(dev.cpu(), cpu)
    assert torch.equal(torch.clamp((dev + 1) / 2, 0, 1).cpu(), torch.clamp((cpu + 1) / 2, 0, 1))
    assert torch.equal(res["trajectories"][0]["manipulated"][0][0].cpu(), cpu)


def test_prompt_editing_against_the_reference_vectors():
    arrays, meta = er.golden()
    case, T = meta["cases"]["prompt"], meta["T"]
    m = golden_model(0.2)
    torch.manual_seed(meta["case_seed"])
    res = prompt_editing.apply_prompt_editing(m, params(T), "a cat", "a dog", config(T), torch.device(DEV))
    assert sorted(res) == ["edited_image", "edited_prompt", "edited_trajectory", "original_image", "original_prompt", "original_trajectory"]
    assert (res["original_prompt"], res["edited_prompt"]) == (case["original_prompt"], case["edited_prompt"])
    for kind in ("original", "edited"):
        check_traj(res[f"{kind}_trajectory"], arrays, f"prompt/{kind}_trajectory", case["timesteps"][kind])
        assert np.allclose(res[f"{kind}_image"].cpu().numpy(), arrays[f"prompt/{kind}_image"], **TOL)
    torch.manual_seed(meta["case_seed"])
    plain = prompt_editing.apply_prompt_editing(m, params(T, False), "a cat", "a dog", config(T), torch.device(DEV))
    assert torch.equal(plain["edited_image"], res["edited_image"])


def test_semantic_directions_are_ten_orthonormal_components():
    T = 4
    m = golden_model(0.2)
    d = latent_manipulation.find_semantic_directions(m, params(T), config(T), torch.device(DEV), num_samples=12)
    assert sorted(d) == sorted(f"pca_{i}" for i in range(10))
    M = torch.stack([d[f"pca_{i}"] for i in range(10)]).double().cpu()
    assert tuple(M.shape) == (10, 768) and torch.allclose(M @ M.T, torch.eye(10, dtype=torch.float64), atol=1e-5)


# ---------------------------------------------------------------------- 6. the sweeps
def sweep_models():
    teacher, students = model(0.3), [model(0.1), model(0.2)]
    handle(0.3, False), handle(0.1, True), handle(0.2, True)
    return teacher, students


def test_inpainting_sweep_cells_equal_single_runs():
    T, S, E = 6, 2, 768
    cfg, dev = config(T), torch.device(DEV)
    teacher, students = sweep_models()
    g = torch.Generator().manual_seed(3)
    images = torch.rand(2, 3, 16, 16, generator=g)
    masks = [rect(256, 1, 4, 11).reshape(16, 16).numpy().astype(np.float64), (torch.rand(1, 16, 16, generator=g) < 0.5).float()]
    out = inpainting_sweep(teacher, students, cfg, images, masks, S, base_seed=42)
    cells = out["cells"].cpu().tolist()
    assert len(cells) == 8 and tuple(out["teacher"][None].shape) == (T + 1, 8, E)
    dp = get_diffusion_params(T, cfg)
    for mi, (m, traj) in enumerate([(teacher, out["teacher"][None])] + [(s, r[None]["trajectory"]) for s, r in zip(students, out["students"])]):
        traj = traj.cpu()
        for b, (i, j, s) in enumerate(cells):
            torch.manual_seed(42 + s)
            mask = masked_inpainting.normalize_mask(masks[j], 3, dev)
            _, single = masked_inpainting.inpaint_with_trajectory(m, dp, images[i:i + 1].to(dev), mask, cfg, dev)
            got = torch.stack([x.reshape(E) for x, _ in single]).cpu()
            assert np.array_equal(traj[:T, b].numpy(), got.numpy()), (mi, i, j, s)
    # hole statistics of teacher against each student, against numpy float64
    mask, known = out["mask"].cpu().numpy(), out["known"].cpu().numpy()
    mr, kr = out["mask_row"].cpu().numpy(), out["known_row"].cpu().numpy()
    X = out["teacher"][None][:T].cpu().numpy()
    for r in out["students"]:
        want = _hole_ref(X, r[None]["trajectory"][:T].cpu().numpy(), mask[mr][None], known[kr][None]).transpose(1, 0, 2)
        got = r[None]["hole"].cpu().numpy()
        assert got.shape == (8, T, 4)
        ok = want > 0
        assert ok.any() and (np.abs(got[ok] - want[ok]) / want[ok]).max() <= 1e-12
        assert (got[~ok] == 0).all()                         # binary masks: nothing differs outside the hole
        assert tuple(r[None]["sums"].shape) == (8, T, 4) and tuple(r[None]["w1"].shape) == (8, T)
        sums, w1 = engine.device_pair_metrics(out["teacher"][None][:T].contiguous(), r[None]["trajectory"][:T].contiguous())
        assert torch.equal(sums, r[None]["sums"]) and torch.equal(w1, r[None]["w1"])


def test_inpainting_sweep_guidance_scales_share_and_split_loops():
    """scales that do not take the two-pass branch share one loop; a guided scale runs the masked CFG loop, whose cells do
    not depend on the batch either (the one-cell sweep of the same image, mask and sample gives the same bits)"""
    T, S = 6, 2
    cfg = config(T)
    teacher, students = sweep_models()
    g = torch.Generator().manual_seed(5)
    images = torch.rand(2, 3, 16, 16, generator=g)
    masks = [rect(256, 1, 3, 12).reshape(16, 16), rect(256, 1, 6, 14).reshape(1, 16, 16)]
    out = inpainting_sweep(teacher, students[:1], cfg, images, masks, S, guidance_scales=(None, 1.0, 3.0))
    assert out["teacher"][None] is out["teacher"][1.0] and out["students"][0][None]["trajectory"] is out["students"][0][1.0]["trajectory"]
    assert not torch.equal(out["teacher"][3.0], out["teacher"][None])
    one = inpainting_sweep(teacher, students[:1], cfg, images[1:], masks[1:], 1, guidance_scales=(3.0, None))
    b = out["cells"].cpu().tolist().index([1, 1, 0])
    for gs in (None, 3.0):
        assert torch.equal(one["teacher"][gs][:, 0], out["teacher"][gs][:, b]), gs
        assert torch.equal(one["students"][0][gs]["trajectory"][:, 0], out["students"][0][gs]["trajectory"][:, b]), gs
        assert torch.equal(one["students"][0][gs]["hole"][0], out["students"][0][gs]["hole"][b]), gs
        hole = out["mask"][1] == 0                           # the known region, under guidance too
        assert torch.equal(out["teacher"][gs][:, b][:, hole], out["known"][1][hole].expand(T + 1, -1)), gs


def test_manipulation_sweep_cells_equal_single_runs():
    T, S, E = 6, 2, 768
    cfg, dev = config(T), torch.device(DEV)
    teacher, students = sweep_models()
    g = torch.Generator().manual_seed(9)
    directions = torch.nn.functional.normalize(torch.randn(2, E, generator=g), dim=1)
    strengths = [2.0, -0.75]
    out = manipulation_sweep(teacher, students, cfg, directions, strengths, S, base_seed=42)
    cells = out["cells"].cpu().tolist()
    assert len(cells) == 8
    dp = get_diffusion_params(T, cfg)
    for mi, (m, res) in enumerate([(teacher, out["teacher"])] + list(zip(students, out["students"]))):
        man, orig, shift = res["manipulated"].cpu(), res["original"].cpu(), res["shift"].cpu()
        for b, (d, k, s) in enumerate(cells):
            torch.manual_seed(42 + s)
            _, latent, t_orig = latent_manipulation.generate_image_with_latents(m, dp, cfg, dev)
            _, t_man = latent_manipulation.manipulate_latent(m, dp, latent, directions[d].to(dev), strengths[k], cfg, dev)
            assert np.array_equal(orig[:T, s].numpy(), torch.stack([x.reshape(E) for x, _ in t_orig]).cpu().numpy()), (mi, s)
            assert np.array_equal(man[:T // 2 + 1, b].numpy(), torch.stack([x.reshape(E) for x, _ in t_man]).cpu().numpy()), (mi, d, k, s)
            want = torch.linalg.vector_norm(t_man[-1][0].reshape(E) - latent.reshape(E)).item()
            assert abs(shift[b].item() - want) <= 1e-5 * want
    for r in out["students"]:
        assert tuple(r["sums"].shape) == (8, T // 2 + 1, 4) and tuple(r["w1"].shape) == (8, T // 2 + 1)
