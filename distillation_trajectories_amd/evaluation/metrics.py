"""Trajectory divergence (reference evaluation/metrics.py:118-183) on the HIP metric kernels, FID (:51-116) and LPIPS
(:22-49).

Distances, cosine similarities and path lengths come from two device reductions (dt_pair_stats, dt_traj_metrics)
over the stacked trajectories instead of 3 x len python loops of ``torch.norm(...).item()`` / sklearn calls.
``compute_fid`` runs the InceptionV3 features on the device with user-supplied weights (``weights=`` or
``DT_INCEPTION_WEIGHTS``).  ``compute_lpips`` runs LPIPS v0.1 (net='alex') on the device, likewise with user-supplied
weights (``weights=`` or ``DT_LPIPS_WEIGHTS``).
"""
import numpy as np
import torch
from scipy.linalg import sqrtm

from .. import engine, lpips
from ..analysis.metrics.fid_score import InceptionModel, calculate_fid_device, extract_features, stats_mode
from ..analysis.metrics.trajectory_metrics import _metrics_device, _stack_on_device


def _as_batch(images):
    return torch.cat(list(images)) if isinstance(images, (list, tuple)) else images


class LPIPSModel:
    """LPIPS v0.1 with net='alex' on ``device``: ``weights`` is a state dict of ``lpips.LPIPS(net='alex')`` or its path,
    or the pair (torchvision AlexNet state dict, the lpips package's alex.pth) as mappings, paths or
    ``"alexnet.pth,alex.pth"`` (default: ``$DT_LPIPS_WEIGHTS``).  ``handle`` is the device handle (lpips.LPIPSHandle)."""

    def __init__(self, device, weights=None):
        self.device = torch.device(device)
        self.handle = lpips.LPIPSHandle(lpips.read_weights(weights), self.device)


def lpips_distances(images1, images2, model, in_scale=2.0, in_shift=-1.0, batch_size=256, per_layer=False):
    """LPIPS between images1[i] and images2[i] ([N, 3, H, W] each; images1 may hold ONE image, compared with every image
    of images2), ``batch_size`` pairs per launch sequence: the device tensor [N], or [N, 5] (the five layer terms, whose
    sum is the distance) with ``per_layer``.  ``in_scale * x + in_shift`` is applied first: the default (2, -1) maps
    [0, 1] as compute_lpips does, (1, 0) takes [-1, 1] as it is.  A pair's value does not depend on the batching."""
    lpips.check_images(images1)
    lpips.check_images(images2)
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if tuple(images1.shape[2:]) != tuple(images2.shape[2:]) or images1.shape[0] not in (1, images2.shape[0]):
        raise ValueError(f"images1 {tuple(images1.shape)} and images2 {tuple(images2.shape)} do not pair up: the same size, "
                         "and one image or as many in images1")
    h = model.handle
    N, shared = images2.shape[0], images1.shape[0] == 1 and images2.shape[0] > 1
    H, W = images2.shape[2:]
    out = torch.empty(N, lpips.N_LAYERS if per_layer else 1, dtype=torch.float32, device=h.device)
    p_shared = h.features(images1, in_scale, in_shift) if shared else None
    for i in range(0, N, batch_size):
        p1 = h.features(images2[i:i + batch_size], in_scale, in_shift)
        p0 = p_shared if shared else h.features(images1[i:i + batch_size], in_scale, in_shift)
        res = h.distance(p0, p1, H, W, per_layer=per_layer)
        out[i:i + batch_size] = res[1] if per_layer else res[:, None]
    return out if per_layer else out[:, 0]


def compute_lpips(image1, image2, device, weights=None, model=None):
    """Reference :22-49: the LPIPS distance (a Python float, lower is more similar) between two images in [0, 1],
    [1, 3, H, W] or [3, H, W], mapped by 2x - 1 as the reference does.  ``weights`` / ``model``: an LPIPSModel to reuse,
    else one is built on ``device`` from ``weights`` (default ``$DT_LPIPS_WEIGHTS``); without weights this raises
    FileNotFoundError -- the reference's placeholder 0.5 is not reproduced.  More than one image per argument raises:
    the reference's ``.item()`` only works for one; use ``lpips_distances``."""
    a = image1[None] if isinstance(image1, torch.Tensor) and image1.dim() == 3 else image1
    b = image2[None] if isinstance(image2, torch.Tensor) and image2.dim() == 3 else image2
    lpips.check_images(a)
    lpips.check_images(b)
    if a.shape[0] != 1 or b.shape[0] != 1:
        raise ValueError(f"compute_lpips takes one image per argument (the reference's .item()), got {a.shape[0]} and "
                         f"{b.shape[0]}; use lpips_distances for batches")
    if model is None:
        model = LPIPSModel(device, weights)
    return lpips_distances(a, b, model).item()


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
