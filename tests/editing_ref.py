"""Torch-CPU restatement of the three editing loops (editing/masked_inpainting.py, latent_manipulation.py,
prompt_editing.py of the reference) on ``oracle.unet_ref``'s forward, written from the algorithm:

  for t = t_first .. 0: record (x, t); eps = model(x, [t]); for t > 0: x' = (c1 x - c2 eps) + sigma z with one randn_like
  draw; inpainting then keeps the known region, x = m x' + (1 - m) k.  The image is clamp((x + 1) / 2, 0, 1).

Every draw comes from the torch CPU global generator in the reference's order; ``load_case`` / ``golden`` read
tests/golden/reference_vectors_editing.{npz,json} once for every test module that needs them.
"""
import functools
import json
import os

import numpy as np
import torch

from oracle import sampler_ref, unet_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPE = (1, 3, 16, 16)


@functools.lru_cache(maxsize=None)
def golden():
    """(arrays, meta) of the reference vectors; arrays must not be modified"""
    with np.load(os.path.join(GOLDEN, "reference_vectors_editing.npz")) as z:
        arrays = {k: z[k] for k in z.files}
    for a in arrays.values():
        a.setflags(write=False)
    with open(os.path.join(GOLDEN, "reference_vectors_editing.json")) as f:
        return arrays, json.load(f)


def eps_fn(sd):
    return lambda x, t: unet_ref.unet_forward(sd, x, torch.tensor([t]), None)


def loop(eps, x, t_first, coef, mask=None, known=None):
    """(final x, [(state, t)]) of one loop from t_first; coef = sampler_ref.engine_coefficients(T)"""
    traj = []
    for t in range(t_first, -1, -1):
        traj.append((x.clone(), t))
        e = eps(x, t)
        if t > 0:
            z = torch.randn_like(x)
            xn = coef[t, 0] * x - coef[t, 1] * e
            xn = xn + coef[t, 2] * z
            x = xn if mask is None else mask * xn + (1 - mask) * known
    return x, traj


def image_of(x):
    return torch.clamp((x + 1) / 2, 0, 1)


def normalize_mask(mask, channels=3):
    if not isinstance(mask, torch.Tensor):
        mask = torch.tensor(mask).float()
    while mask.dim() < 4:
        mask = mask.unsqueeze(0)
    return mask.expand(-1, channels, -1, -1)


def random_mask(h, w, lo=0.2, hi=0.5):
    m = np.zeros((h, w))
    mh, mw = int(np.random.uniform(lo, hi) * h), int(np.random.uniform(lo, hi) * w)
    y, x = np.random.randint(0, h - mh), np.random.randint(0, w - mw)
    m[y:y + mh, x:x + mw] = 1
    return m


def inpaint(sd, T, original, mask):
    """apply_masked_inpainting: dict(original_image, inpainted_image, mask, trajectory)"""
    eps, coef = eps_fn(sd), sampler_ref.engine_coefficients(T)
    if original is None:
        torch.manual_seed(torch.randint(0, 10000, (1,)).item())
        original = image_of(loop(eps, torch.randn(*SHAPE), T - 1, coef)[0])
    if mask is None:
        mask = random_mask(16, 16)
    mask = normalize_mask(mask)
    x = torch.randn(*SHAPE)
    known = 2 * original - 1
    x = mask * x + (1 - mask) * known
    x, traj = loop(eps, x, T - 1, coef, mask, known)
    return dict(original_image=original, inpainted_image=image_of(x), mask=mask, trajectory=traj)


def manipulate(sd, T, strength, num_samples):
    """apply_latent_manipulation with a 'random' direction"""
    eps, coef = eps_fn(sd), sampler_ref.engine_coefficients(T)
    seed = torch.randint(0, 10000, (1,)).item()
    direction = torch.randn(768)
    direction = direction / torch.norm(direction)
    out = dict(direction=direction, original_images=[], manipulated_images=[], trajectories=[])
    for i in range(num_samples):
        torch.manual_seed(seed + i)
        latent, t_orig = loop(eps, torch.randn(*SHAPE), T - 1, coef)
        x, t_man = loop(eps, latent + strength * direction.reshape(latent.shape), T // 2, coef)
        out["original_images"].append(image_of(latent))
        out["manipulated_images"].append(image_of(x))
        out["trajectories"].append(dict(original=t_orig, manipulated=t_man))
    return out


def prompt(sd, T):
    """apply_prompt_editing: the second 'prompt' is seed + 1"""
    eps, coef = eps_fn(sd), sampler_ref.engine_coefficients(T)
    seed = torch.randint(0, 10000, (1,)).item()
    out = {}
    for kind, s in (("original", seed), ("edited", seed + 1)):
        torch.manual_seed(s)
        x, traj = loop(eps, torch.randn(*SHAPE), T - 1, coef)
        out[f"{kind}_image"], out[f"{kind}_trajectory"] = image_of(x), traj
    return out


def stack(traj):
    return torch.stack([x for x, _ in traj]).numpy(), [t for _, t in traj]
