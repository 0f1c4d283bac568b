"""Drop-in for the reference's ``editing/prompt_editing.py`` on the HIP path: the same signatures and return dicts.  The
reference has no text conditioning: its "edited prompt" is a second seed (seed + 1), and that is what is mirrored."""
import os

import numpy as np
import torch

from . import _loop


def apply_prompt_editing(model, diffusion_params, original_prompt, edited_prompt, config, device, record_trajectory=True):
    """reference :11-64: a ``torch.randint`` seed; the original image under it, the edited image under seed + 1."""
    model.eval()
    seed = torch.randint(0, 10000, (1,)).item()
    torch.manual_seed(seed)
    original_image, original_trajectory = generate_image_with_trajectory(model, diffusion_params, config, device)
    torch.manual_seed(seed + 1)
    edited_image, edited_trajectory = generate_image_with_trajectory(model, diffusion_params, config, device)
    result = {"original_image": original_image, "edited_image": edited_image, "original_prompt": original_prompt,
              "edited_prompt": edited_prompt}
    if record_trajectory:
        result["original_trajectory"] = original_trajectory
        result["edited_trajectory"] = edited_trajectory
    return result


def generate_image_with_trajectory(model, diffusion_params, config, device):
    """(image in [0, 1], [(state, t)] for t = T-1 .. 0) (reference :66-120)."""
    T, coefs = _loop.schedule(diffusion_params)
    shape = (1, config.channels, config.image_size, config.image_size)
    x0, steps = _loop.draw_loop(shape, T - 1)
    traj = _loop.run_single(model, x0, steps, T - 1, coefs, config, device)
    return _loop.to_image(traj[T - 1].reshape(shape)).to(device), _loop.as_trajectory(traj, T - 1, config, device)


def visualize_prompt_editing(result, output_dir, size_factor=None):
    """``prompt_editing_comparison.npz`` (both images and prompts) and, with trajectories, both state stacks with their
    timesteps in ``trajectories/prompt_trajectories.npz`` in place of the figures (reference :122-)."""
    os.makedirs(output_dir, exist_ok=True)
    np.savez(os.path.join(output_dir, "prompt_editing_comparison.npz"), original=result["original_image"].cpu().numpy(),
             edited=result["edited_image"].cpu().numpy(), original_prompt=str(result["original_prompt"]),
             edited_prompt=str(result["edited_prompt"]), size_factor=np.nan if size_factor is None else size_factor)
    if "original_trajectory" in result:
        traj_dir = os.path.join(output_dir, "trajectories")
        os.makedirs(traj_dir, exist_ok=True)
        arrays = {}
        for kind in ("original", "edited"):
            traj = result[f"{kind}_trajectory"]
            arrays[kind] = torch.cat([x for x, _ in traj]).cpu().numpy()
            arrays[f"{kind}_timesteps"] = np.array([t for _, t in traj])
        np.savez(os.path.join(traj_dir, "prompt_trajectories.npz"), **arrays)
