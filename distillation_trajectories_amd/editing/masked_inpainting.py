"""Drop-in for the reference's ``editing/masked_inpainting.py`` on the HIP path: the same signatures and return dicts.

The loop (see ``_loop``) runs as one ``dt_sample_trajectory_masked`` call: the known-region blend
``x = mask * x_updated + (1 - mask) * original_scaled`` (:218) is part of the reverse step's kernel, the start state
(:178-181) is ``dt_edit_start``.  ``visualize_*`` write npz files in place of the figures.
"""
import os

import numpy as np
import torch

from . import _loop


def normalize_mask(mask, channels, device):
    """The mask as the reference shapes it (:52-62): float32 [1, channels, H, W] (an expanded view) on ``device`` from a
    2-D / 3-D / 4-D array or tensor."""
    if not isinstance(mask, torch.Tensor):
        mask = torch.tensor(mask, device=device).float()
    if len(mask.shape) == 2:
        mask = mask.unsqueeze(0).unsqueeze(0)
    elif len(mask.shape) == 3:
        mask = mask.unsqueeze(0)
    return mask.expand(-1, channels, -1, -1)


def apply_masked_inpainting(model, diffusion_params, original_image, mask, config, device, record_trajectory=True):
    """reference :11-78.  ``original_image`` None: an image is generated under a seed drawn with ``torch.randint``;
    ``mask`` None: ``create_random_mask`` (NumPy's global generator)."""
    model.eval()
    if original_image is None:
        seed = torch.randint(0, 10000, (1,)).item()
        torch.manual_seed(seed)
        original_image, _ = generate_image(model, diffusion_params, config, device)
    if mask is None:
        mask = create_random_mask(config.image_size, config.image_size)
    mask = normalize_mask(mask, config.channels, device)
    inpainted_image, trajectory = inpaint_with_trajectory(model, diffusion_params, original_image, mask, config, device)
    result = {"original_image": original_image, "inpainted_image": inpainted_image, "mask": mask}
    if record_trajectory:
        result["trajectory"] = trajectory
    return result


def create_random_mask(height, width, min_size=0.2, max_size=0.5):
    """A random rectangle of ones in a [height, width] float64 array of zeros (reference :80-107): two ``uniform`` draws for
    the size, two ``randint`` draws for the position, from NumPy's global generator in that order."""
    mask = np.zeros((height, width))
    mask_h = int(np.random.uniform(min_size, max_size) * height)
    mask_w = int(np.random.uniform(min_size, max_size) * width)
    mask_y = np.random.randint(0, height - mask_h)
    mask_x = np.random.randint(0, width - mask_w)
    mask[mask_y:mask_y + mask_h, mask_x:mask_x + mask_w] = 1
    return mask


def generate_image(model, diffusion_params, config, device):
    """(image in [0, 1], None): the plain loop from noise, no trajectory kept (reference :109-157)."""
    T, coefs = _loop.schedule(diffusion_params)
    shape = (1, config.channels, config.image_size, config.image_size)
    x0, steps = _loop.draw_loop(shape, T - 1)
    traj = _loop.run_single(model, x0, steps, T - 1, coefs, config, device)
    return _loop.to_image(traj[T - 1].reshape(shape)).to(device), None


def inpaint_with_trajectory(model, diffusion_params, original_image, mask, config, device):
    """(inpainted image in [0, 1], [(state, t)] for t = T-1 .. 0) (reference :159-224); ``mask`` is [1, C, H, W]."""
    T, coefs = _loop.schedule(diffusion_params)
    shape = (1, config.channels, config.image_size, config.image_size)
    x0, steps = _loop.draw_loop(shape, T - 1)
    m = mask.expand(shape).float().contiguous()
    traj = _loop.run_single(model, x0, steps, T - 1, coefs, config, device, mask=m, image=original_image.float())
    return _loop.to_image(traj[T - 1].reshape(shape)).to(device), _loop.as_trajectory(traj, T - 1, config, device)


def _sample_indices(trajectory):
    return np.linspace(0, len(trajectory) - 1, min(5, len(trajectory)), dtype=int)


def visualize_inpainting(result, output_dir, size_factor=None):
    """``inpainting_comparison.npz`` (original, mask, inpainted) in place of the figure (reference :226-270)."""
    os.makedirs(output_dir, exist_ok=True)
    np.savez(os.path.join(output_dir, "inpainting_comparison.npz"), original=result["original_image"].cpu().numpy(),
             mask=result["mask"].cpu().numpy(), inpainted=result["inpainted_image"].cpu().numpy(),
             size_factor=np.nan if size_factor is None else size_factor)
    if "trajectory" in result:
        visualize_inpainting_trajectory(result["trajectory"], result["mask"], output_dir, size_factor)


def visualize_inpainting_trajectory(trajectory, mask, output_dir, size_factor=None):
    """``trajectories/inpainting_trajectory.npz``: the (at most five) states the reference's figure shows, as images in
    [0, 1], with their timesteps and the mask (reference :272-353)."""
    traj_dir = os.path.join(output_dir, "trajectories")
    os.makedirs(traj_dir, exist_ok=True)
    idx = _sample_indices(trajectory)
    images = torch.stack([_loop.to_image(trajectory[i][0])[0] for i in idx]).cpu().numpy()
    np.savez(os.path.join(traj_dir, "inpainting_trajectory.npz"), images=images, timesteps=np.array([trajectory[i][1] for i in idx]),
             mask=mask.cpu().numpy(), size_factor=np.nan if size_factor is None else size_factor)
