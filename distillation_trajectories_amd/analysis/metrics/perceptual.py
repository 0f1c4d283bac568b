"""Perceptual distance between teacher and student trajectories: LPIPS (v0.1, net='alex') per timestep, per student and
per guidance scale, on the states the grid already holds on the device.  Only the distances leave the device."""
import torch

from ... import engine, lpips
from ...evaluation.metrics import LPIPSModel


def state_indices(n_states, every):
    """Every ``every``-th state index, plus the last."""
    if every < 1:
        raise ValueError(f"every must be >= 1, got {every}")
    idx = list(range(0, n_states, every))
    if idx[-1] != n_states - 1:
        idx.append(n_states - 1)
    return idx


def _images(states, C, H, resize):
    """[n, E] trajectory states -> [n, C, h, w] images, resized (align_corners=True bilinear) when asked."""
    x = states.reshape(-1, C, H, H)
    return engine.resize_bilinear(x, resize) if resize is not None else x.contiguous()


def lpips_sweep(teacher_model, student_models, config, guidance_scales, num_samples, weights=None, every=1, resize=None,
                model=None):
    """LPIPS between the teacher's and each student's state at the same step of the same sample, for a whole grid cell:
    ``sample_grid`` for each model exactly as ``pca_sweep`` runs it (sample s starts from seed 42 + s), the teacher's
    feature packs once per guidance scale for every ``every``-th state plus the last, then ONE distance launch per scale
    that shares them among all students.  States go in as they are ([-1, 1], map (1, 0)).  ``resize=(H, W)`` first resizes
    them with ``engine.resize_bilinear`` (AlexNet needs at least 31 x 31); without it an image size below 31 raises
    ValueError before anything is sampled.  Returns numpy ``lpips`` [n_students][n_scales][n_states][S], ``per_layer``
    [..., 5] and ``states`` (the state indices).  ``weights`` as LPIPSModel takes them (default ``$DT_LPIPS_WEIGHTS``)."""
    from ..trajectory_engine import sample_grid
    from ...synthetic import noise_table
    C, H, T, S = config.channels, config.image_size, config.timesteps, num_samples
    size = (int(resize[0]), int(resize[1])) if resize is not None else (H, H)
    lpips.check_size(*size)
    if C != 3:
        raise ValueError(f"LPIPS: images must have 3 channels, got {C}")
    idx = state_indices(T + 1, every)
    students, scales = list(student_models), list(guidance_scales)
    if not students:
        raise ValueError("lpips_sweep needs at least one student")
    device = next(teacher_model.parameters()).device
    if model is None:
        model = LPIPSModel(device, weights)
    h = model.handle
    G, n = len(students), len(idx) * S
    with torch.cuda.device(device):
        table = noise_table(42, S + T - 1, (1, C, H, H)).reshape(S + T - 1, -1).to(device)
        t_grid = sample_grid(engine.UNetHandle.for_module(teacher_model), table, 0, S, T, scales, H, H)
        s_grids = [sample_grid(engine.UNetHandle.for_module(m), table, 0, S, T, scales, H, H) for m in students]
        F = lpips.feature_floats(*size)
        dist, layers = [], []
        for gs in scales:
            p0 = h.features(_images(t_grid[gs][idx], C, H, resize))
            p1 = torch.empty(G, n, F, dtype=torch.float32, device=device)
            for g, grid in enumerate(s_grids):
                h.features(_images(grid[gs][idx], C, H, resize), out=p1[g])
            d, per = h.distance_many(p0, p1, size[0], size[1], per_layer=True)
            dist.append(d.view(G, len(idx), S))
            layers.append(per.view(G, len(idx), S, lpips.N_LAYERS))
        return {"lpips": torch.stack(dist, dim=1).cpu().numpy(), "per_layer": torch.stack(layers, dim=1).cpu().numpy(),
                "states": idx}
