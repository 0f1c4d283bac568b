"""Trajectory divergence (reference evaluation/metrics.py:118-183) on the HIP metric kernels, and FID (:51-116).

Distances, cosine similarities and path lengths come from two device reductions (dt_pair_stats, dt_traj_metrics)
over the stacked trajectories instead of 3 x len python loops of ``torch.norm(...).item()`` / sklearn calls.
``compute_fid`` runs the InceptionV3 features on the device with user-supplied weights (``weights=`` or
``DT_INCEPTION_WEIGHTS``).  LPIPS is not provided: it needs a pretrained network of its own.
"""
import numpy as np
import torch
from scipy.linalg import sqrtm

from .. import engine
from ..analysis.metrics.fid_score import InceptionModel, calculate_fid_device, extract_features, stats_mode
from ..analysis.metrics.trajectory_metrics import _metrics_device, _stack_on_device


def _as_batch(images):
    return torch.cat(list(images)) if isinstance(images, (list, tuple)) else images


def compute_fid(real_images, generated_images, device, batch_size=8, weights=None, stats=None):
    """Reference :51-116: FID between two image sets (lists of [1, 3, H, W] tensors, or [N, 3, H, W] tensors), taken
    as given (no (x + 1) / 2), with the reference's arithmetic.  ``weights``: torchvision's Inception3 state dict or
    its path (default ``$DT_INCEPTION_WEIGHTS``).  ``stats``: "host" (the default, unless ``$DT_FID_STATS`` says
    otherwise) or "device": the features stay on the device and the distance is taken there (``calculate_fid_device``)."""
    mode = stats_mode(stats)
    real, gen = _as_batch(real_images), _as_batch(generated_images)
    inception = InceptionModel(device, weights)
    if mode == "device":
        return calculate_fid_device(extract_features(real, inception, batch_size=batch_size),
                                    extract_features(gen, inception, batch_size=batch_size))
    real_features = extract_features(real, inception, batch_size=batch_size).cpu().numpy()
    gen_features = extract_features(gen, inception, batch_size=batch_size).cpu().numpy()
    mu_real = np.mean(real_features, axis=0)
    sigma_real = np.cov(real_features, rowvar=False)
    mu_gen = np.mean(gen_features, axis=0)
    sigma_gen = np.cov(gen_features, rowvar=False)
    diff = mu_real - mu_gen
    covmean = sqrtm(sigma_real.dot(sigma_gen))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma_real + sigma_gen - 2 * covmean)


def compute_trajectory_divergence(trajectory1, trajectory2):
    """Same keys as the reference: distances, similarities, avg/max distance, avg/min similarity, length_ratio.
    Trajectories are lists of (image, timestep) pairs (the reference indexes ``item[0]`` unconditionally)."""
    im1 = [item[0] for item in trajectory1]
    im2 = [item[0] for item in trajectory2]
    device = im1[0].device if im1[0].is_cuda else _metrics_device()
    X, Y = _stack_on_device(im1, device), _stack_on_device(im2, device)
    n = min(len(im1), len(im2))
    f32 = np.float32
    stats = engine.device_pair_stats(X[:n].contiguous(), Y[:n].contiguous())[0].cpu().numpy().astype(f32)   # [n,5]
    sums = engine.device_metric_sums(X, Y)[0].cpu().numpy().astype(f32)
    distances = [float(np.sqrt(stats[i, 0])) for i in range(n)]
    sims = []
    for i in range(n):
        nx, ny = np.sqrt(stats[i, 3]), np.sqrt(stats[i, 4])
        nx = nx if nx > 0 else f32(1.0)            # sklearn normalises zero rows with a unit scale
        ny = ny if ny > 0 else f32(1.0)
        sims.append(f32(stats[i, 2] / (nx * ny)))
    length1 = 0
    for i in range(1, len(im1)):
        length1 += float(np.sqrt(sums[i, 1]))
    length2 = 0
    for i in range(1, len(im2)):
        length2 += float(np.sqrt(sums[i, 2]))
    return {
        "distances": distances,
        "similarities": sims,
        "avg_distance": np.mean(distances),
        "max_distance": np.max(distances),
        "avg_similarity": np.mean(sims),
        "min_similarity": np.min(sims),
        "length_ratio": length2 / length1 if length1 > 0 else float("inf"),
    }
