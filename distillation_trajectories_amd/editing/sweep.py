"""Batched editing sweeps: what the B = 1 loops of ``masked_inpainting`` and ``latent_manipulation`` compute for many cells,
in one sampler loop per model, with the teacher run once and shared by every student.

A cell's numbers are those of the same cell run alone: the kernels treat batch rows independently, images, masks and noise
reach a row through row tables (nothing is replicated), and sample s draws its noise exactly as a single run seeded with
``base_seed + s`` does (``torch.manual_seed``, one start draw, one draw per t > 0 -- then, for manipulation, one draw per
t > 0 of the re-run).  The global generator is left where the last sample's draws leave it.
"""
import torch

from .. import engine
from . import _loop
from ..utils.diffusion import get_diffusion_params
from .masked_inpainting import normalize_mask


def _scales(guidance_scales):
    """{scale: key of the loop that serves it}: every scale that does not take the two-pass branch shares one loop"""
    return {gs: (gs if gs is not None and gs > 1.0 else None) for gs in guidance_scales}


def _sample_noise(base_seed, S, shape, t_first, t_rerun=0):
    """(start rows [S, E], step table [S * t_first, E], re-run step table [S * t_rerun, E]) of samples 0 .. S-1"""
    starts, steps, rerun = [], [], []
    for s in range(S):
        torch.manual_seed(base_seed + s)
        x0, st = _loop.draw_loop(shape, t_first)
        starts.append(x0); steps.append(st)
        rerun.append(_loop.draw_steps(shape, t_rerun))
    return torch.cat(starts), torch.cat(steps), torch.cat(rerun)


def inpainting_sweep(teacher, students, config, images, masks, num_samples, guidance_scales=(None,), base_seed=42):
    """Inpaint every (image, mask, sample) cell with the teacher and every student.

    images [n_img, C, H, W] in [0, 1]; masks: a sequence of 2-D / 3-D masks (``normalize_mask``); sample s is seeded with
    ``base_seed + s``.  Cell (i, j, s) is batch row (i * n_mask + j) * S + s.  Returns a dict of device tensors:
      cells [B, 3] (int64: image, mask, sample), mask [n_mask, E], known [n_img, E], mask_row, known_row [B] int32,
      teacher {scale: trajectory [T + 1, B, E]} (slots 0 .. T-1 are the recorded states),
      students [{scale: {trajectory, sums [B, T, 4], w1 [B, T]  (``engine.device_pair_metrics`` of the T recorded states,
                         teacher against student), hole [B, T, 4]  (``engine.device_masked_pair_stats``)}}].
    """
    dev = next(teacher.parameters()).device
    C, H, T, S = config.channels, config.image_size, config.timesteps, num_samples
    E, shape = C * H * H, (1, C, H, H)
    images = images.reshape(-1, E).float().to(dev)
    mask = torch.cat([normalize_mask(m, C, dev).to(dev).float().reshape(1, E) for m in masks]).contiguous()
    n_img, n_mask = images.shape[0], mask.shape[0]
    cells = torch.tensor([(i, j, s) for i in range(n_img) for j in range(n_mask) for s in range(S)])
    B = cells.shape[0]
    known_row, mask_row = (cells[:, k].to(torch.int32).to(dev) for k in (0, 1))
    start_row = cells[:, 2].to(torch.int32).to(dev)
    step_row = (cells[:, 2] * (T - 1)).to(torch.int32).to(dev)
    starts, steps, _ = _sample_noise(base_seed, S, shape, T - 1)
    starts, steps = starts.to(dev), steps.to(dev)
    coefs = _loop.schedule(get_diffusion_params(T, config))[1]
    keys = _scales(guidance_scales)

    def run(model):
        h, out = engine.UNetHandle.for_module(model), {}
        for key in dict.fromkeys(keys.values()):
            traj = torch.empty(T + 1, B, E, dtype=torch.float32, device=dev)
            known, _ = engine.edit_start(images, starts, mask, B, img_row=known_row, z_row=start_row, mask_row=mask_row, x_out=traj[0])
            out[key] = _loop.reverse_loop(h, traj, T - 1, coefs, steps, H, H, z_row=step_row, mask=mask, known=known,
                                          mask_row=mask_row, known_row=known_row, guidance_scale=key), known
        return out

    with torch.cuda.device(dev):
        t_out = run(teacher.eval())
        known = next(iter(t_out.values()))[1]
        per_student = []
        for m in students:
            s_out, res = run(m.eval()), {}
            for gs, key in keys.items():
                X, Y = t_out[key][0][:T], s_out[key][0][:T]
                sums, w1 = engine.device_pair_metrics(X, Y)
                res[gs] = dict(trajectory=s_out[key][0], sums=sums, w1=w1,
                               hole=engine.device_masked_pair_stats(X, Y, mask, known, mask_row, known_row))
            per_student.append(res)
    return dict(cells=cells.to(dev), mask=mask, known=known, mask_row=mask_row, known_row=known_row,
                teacher={gs: t_out[key][0] for gs, key in keys.items()}, students=per_student)


def manipulation_sweep(teacher, students, config, directions, strengths, num_samples, base_seed=42):
    """Every (direction, strength, sample) manipulation with the teacher and every student.

    Per model the S originals run once (one loop of batch S); then every cell's ``latent + strength * direction`` is re-run
    from T // 2 in one loop of batch D * K * S.  directions [D, E] (or [D, C, H, W]); cell (d, k, s) is batch row
    (d * K + k) * S + s.  Returns a dict of device tensors:
      cells [B, 3] (int64: direction, strength, sample),
      teacher {original [T + 1, S, E], manipulated [T // 2 + 2, B, E], shift [B]},
      students [{original, manipulated, shift, sums [B, n, 4], w1 [B, n]}]     n = T // 2 + 1 recorded states
    ``shift`` is ||manipulated_final - original_final|| (fp32 norm of the fp32 difference) per cell; ``sums`` / ``w1`` are
    ``engine.device_pair_metrics`` of the manipulated trajectories, teacher against student.
    """
    dev = next(teacher.parameters()).device
    C, H, T, S = config.channels, config.image_size, config.timesteps, num_samples
    E, shape, half = C * H * H, (1, C, H, H), T // 2
    directions = directions.reshape(directions.shape[0], E).float().to(dev)
    D, K = directions.shape[0], len(strengths)
    cells = torch.tensor([(d, k, s) for d in range(D) for k in range(K) for s in range(S)])
    B = cells.shape[0]
    starts, steps, rerun = (t.to(dev) for t in _sample_noise(base_seed, S, shape, T - 1, half))
    step_row = (torch.arange(S) * (T - 1)).to(torch.int32).to(dev)
    rerun_row = (cells[:, 2] * half).to(torch.int32).to(dev)
    coefs = _loop.schedule(get_diffusion_params(T, config))[1]

    def run(model):
        h = engine.UNetHandle.for_module(model)
        orig = torch.empty(T + 1, S, E, dtype=torch.float32, device=dev)
        orig[0].copy_(starts)
        _loop.reverse_loop(h, orig, T - 1, coefs, steps, H, H, z_row=step_row)
        man = torch.empty(half + 2, B, E, dtype=torch.float32, device=dev)
        for d in range(D):
            for k in range(K):
                r = (d * K + k) * S
                man[0, r:r + S] = orig[T - 1] + strengths[k] * directions[d]         # a product, then a sum, per cell
        _loop.reverse_loop(h, man, half, coefs, rerun, H, H, z_row=rerun_row)
        shift = torch.linalg.vector_norm(man[half] - orig[T - 1].repeat(D * K, 1), dim=1)
        return dict(original=orig, manipulated=man, shift=shift)

    with torch.cuda.device(dev):
        t_out = run(teacher.eval())
        per_student = []
        for m in students:
            res = run(m.eval())
            res["sums"], res["w1"] = engine.device_pair_metrics(t_out["manipulated"][:half + 1], res["manipulated"][:half + 1])
            per_student.append(res)
    return dict(cells=cells.to(dev), teacher=t_out, students=per_student)
