"""Drop-in for the reference's ``editing/latent_manipulation.py`` on the HIP path: the same signatures and return dicts.

``find_semantic_directions`` fits its 10 components with ``TrajectoryPCA`` (exact and deterministic).  The reference calls
sklearn's default solver, which is randomized for these shapes and takes no random_state, so its directions are not
bit-stable from run to run; the exact components are what that solver approximates.
"""
import os

import numpy as np
import torch

from . import _loop


def apply_latent_manipulation(model, diffusion_params, direction, strength, config, device, num_samples=5,
                              record_trajectory=True):
    """reference :12-90: a ``torch.randint`` seed, a random unit direction unless one is given, and per sample i (seed + i)
    an original loop and its manipulated re-run from T // 2."""
    model.eval()
    seed = torch.randint(0, 10000, (1,)).item()
    original_images, manipulated_images, trajectories = [], [], []
    if direction is None or (isinstance(direction, str) and direction == "random"):
        direction = torch.randn(config.channels * config.image_size * config.image_size)
        direction = (direction / torch.norm(direction)).to(device)
    for i in range(num_samples):
        torch.manual_seed(seed + i)
        original_image, original_latents, original_trajectory = generate_image_with_latents(model, diffusion_params, config, device)
        manipulated_image, manipulated_trajectory = manipulate_latent(model, diffusion_params, original_latents, direction,
                                                                      strength, config, device)
        original_images.append(original_image)
        manipulated_images.append(manipulated_image)
        if record_trajectory:
            trajectories.append({"original": original_trajectory, "manipulated": manipulated_trajectory})
    result = {"original_images": original_images, "manipulated_images": manipulated_images, "direction": direction,
              "strength": strength}
    if record_trajectory:
        result["trajectories"] = trajectories
    return result


def generate_image_with_latents(model, diffusion_params, config, device):
    """(image in [0, 1], final latent [1, C, H, W], [(state, t)] for t = T-1 .. 0) (reference :92-149)."""
    T, coefs = _loop.schedule(diffusion_params)
    shape = (1, config.channels, config.image_size, config.image_size)
    x0, steps = _loop.draw_loop(shape, T - 1)
    traj = _loop.run_single(model, x0, steps, T - 1, coefs, config, device)
    final = traj[T - 1].reshape(shape).to(device)
    return _loop.to_image(final), final.clone(), _loop.as_trajectory(traj, T - 1, config, device)


def manipulate_latent(model, diffusion_params, latent, direction, strength, config, device):
    """(image in [0, 1], [(state, t)] for t = T // 2 .. 0) from ``latent + strength * direction`` (reference :151-215)."""
    T, coefs = _loop.schedule(diffusion_params)
    if direction.dim() == 1:
        direction = direction.reshape(latent.shape)
    shape = (1, config.channels, config.image_size, config.image_size)
    steps = _loop.draw_steps(shape, T // 2)
    handle_device = next(model.parameters()).device
    x0 = latent.to(handle_device) + strength * direction.to(handle_device)        # a product, then a sum (no alpha= fusing)
    traj = _loop.run_single(model, x0, steps, T // 2, coefs, config, device)
    return _loop.to_image(traj[T // 2].reshape(shape)).to(device), _loop.as_trajectory(traj, T // 2, config, device)


def find_semantic_directions(model, diffusion_params, config, device, num_samples=100):
    """{"pca_0" .. "pca_9": direction [C*H*W]}: the principal components of the final latents of seeds 0 .. num_samples-1
    (reference :217-258), fitted on the device."""
    from ..analysis.dimensionality.pca import TrajectoryPCA
    latents = []
    for i in range(num_samples):
        torch.manual_seed(i)
        _, latent, _ = generate_image_with_latents(model, diffusion_params, config, device)
        latents.append(latent.reshape(-1))
    pca = TrajectoryPCA(n_components=10)
    pca.fit(torch.stack(latents))
    return {f"pca_{i}": torch.tensor(pca.components_[i], device=device).float() for i in range(10)}


def visualize_latent_manipulation(result, output_dir, size_factor=None):
    """``latent_manipulation_comparison.npz`` (original and manipulated images, direction, strength) and, with
    trajectories, ``trajectories/latent_trajectory_sample_{i}.npz`` in place of the figures (reference :260-)."""
    os.makedirs(output_dir, exist_ok=True)
    np.savez(os.path.join(output_dir, "latent_manipulation_comparison.npz"),
             original=torch.cat(result["original_images"]).cpu().numpy(),
             manipulated=torch.cat(result["manipulated_images"]).cpu().numpy(),
             direction=result["direction"].cpu().numpy(), strength=result["strength"],
             size_factor=np.nan if size_factor is None else size_factor)
    if "trajectories" in result:
        traj_dir = os.path.join(output_dir, "trajectories")
        os.makedirs(traj_dir, exist_ok=True)
        for i, pair in enumerate(result["trajectories"]):
            arrays = {}
            for kind, traj in pair.items():
                arrays[kind] = torch.cat([x for x, _ in traj]).cpu().numpy()
                arrays[f"{kind}_timesteps"] = np.array([t for _, t in traj])
            np.savez(os.path.join(traj_dir, f"latent_trajectory_sample_{i}.npz"), **arrays)
