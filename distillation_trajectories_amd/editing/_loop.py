"""What the three editing modules share: the schedule read from ``diffusion_params``, the noise draws in the reference's
order, and the one reverse loop on the device (editing/masked_inpainting.py:186-219, latent_manipulation.py:112-140 and
:181-209, prompt_editing.py:86-114):

  one pass ``model(x, [t])`` for t = t_first .. 0; the state is recorded BEFORE the update; for t > 0 the ENGINE update runs
  with one ``randn_like`` draw; at t == 0 nothing is updated; the image is ``clamp((x + 1) / 2, 0, 1)``.

RNG contract: every draw comes from the torch CPU global generator, in the reference's order -- one ``randn(1, C, H, W)``
start state, then one draw per t > 0.  The U-Net consumes no random numbers, so the draws of a loop are taken up front,
staged as one table and uploaded once; there is no device RNG.
"""
import torch

from .. import engine
from .._hip import RULE_ENGINE
from ..analysis.trajectory_engine import _plan, engine_coefficients_from_alphas, uses_cfg


def schedule(diffusion_params):
    """(T, [(c1, c2, sigma)] for t = 0 .. T-1).  ``"timesteps"`` and ``"alphas"`` are honoured when present; the dict of
    ``get_diffusion_params`` has neither (the reference's modules raise KeyError on it), so they default to ``len(betas)``
    and ``1 - betas``."""
    betas = diffusion_params["betas"]
    T = int(diffusion_params["timesteps"]) if "timesteps" in diffusion_params else len(betas)
    alphas = diffusion_params["alphas"] if "alphas" in diffusion_params else 1 - betas
    return T, engine_coefficients_from_alphas(alphas, T)


def draw_steps(shape, t_first):
    """[t_first, numel] table of the step noise of a loop from t_first: row i is the draw at t = t_first - i > 0."""
    rows = [torch.randn(*shape).reshape(-1) for _ in range(t_first)]
    n = 1
    for d in shape:
        n *= d
    return torch.stack(rows) if rows else torch.empty(0, n)


def draw_loop(shape, t_first):
    """(start state [1, numel], step table) of a loop that starts from noise: ``randn(shape)``, then ``draw_steps``."""
    x = torch.randn(*shape).reshape(1, -1)
    return x, draw_steps(shape, t_first)


def reverse_loop(handle, traj, t_first, coefs, z, H, W, z_row=None, mask=None, known=None, mask_row=None, known_row=None,
                 guidance_scale=None):
    """Run t = t_first .. 0 in place on traj [t_first + 2, B, E] (slot 0 = the start states): slot i holds the state
    recorded at t = t_first - i, the last slot repeats slot t_first (nothing is updated at t == 0, and the forward whose
    prediction nobody reads is skipped).  Every image reads row ``z_row[b] + i`` of the device table z at step i.  With
    ``mask`` / ``known`` (and their row tables) the known-region blend follows every update.  ``guidance_scale`` > 1 (the
    sweeps only; the reference's editing loops have no guidance) takes trajectory_engine's two-pass CFG branch."""
    order = list(range(t_first, -1, -1))
    cfg = uses_cfg(guidance_scale)
    t_rows, modes, n_pass = _plan(t_first + 1, cfg)
    tb = handle.time_bias(t_rows, modes)
    args = dict(z=z if z is not None and z.numel() else None, z_row=z_row, z_shift=list(range(len(order))),
                w_scalar=float(guidance_scale) if cfg else 1.0)
    cs, noise = [coefs[t] for t in order], [t > 0 for t in order]
    if mask is None:
        return handle.sample(RULE_ENGINE, traj, H, W, tb, n_pass, cs, noise, **args)
    return handle.sample_masked(RULE_ENGINE, traj, H, W, tb, n_pass, cs, noise, mask, known, mask_row, known_row, **args)


def run_single(model, x0, steps, t_first, coefs, config, device, mask=None, image=None):
    """One B = 1 loop from host start state x0 [1, E] (``image`` given: x0 is the noise of the masked start) with the host
    step table ``steps``.  Returns the device trajectory buffer [t_first + 2, 1, E]."""
    h = engine.UNetHandle.for_module(model)
    C, H = config.channels, config.image_size
    E = C * H * H
    traj = torch.empty(t_first + 2, 1, E, dtype=torch.float32, device=h.device)
    z = steps.to(h.device)
    if mask is None:
        traj[0].copy_(x0.reshape(1, E))
        return reverse_loop(h, traj, t_first, coefs, z, H, H)
    m = mask.to(h.device).reshape(1, E).contiguous()
    known, _ = engine.edit_start(image.to(h.device).reshape(1, E), x0.to(h.device).reshape(1, E), m, 1, x_out=traj[0])
    return reverse_loop(h, traj, t_first, coefs, z, H, H, mask=m, known=known)


def to_image(x):
    """clamp((x + 1) / 2, 0, 1), the reference's two ops and a clamp (torch ops on x's device)"""
    return torch.clamp((x + 1) / 2, 0, 1)


def as_trajectory(traj, t_first, config, device):
    """[(state [1, C, H, W], t)] for t = t_first .. 0 from slots 0 .. t_first of a B = 1 trajectory buffer"""
    C, H = config.channels, config.image_size
    states = traj[: t_first + 1].reshape(t_first + 1, 1, C, H, H).to(device)
    return [(states[i], t) for i, t in enumerate(range(t_first, -1, -1))]
