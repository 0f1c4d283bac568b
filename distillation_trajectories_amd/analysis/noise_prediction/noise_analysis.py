"""Teacher-vs-student noise-prediction metrics (reference analysis/noise_prediction/noise_analysis.py).

``predict_noise`` is one U-Net forward on the HIP path; ``calculate_noise_metrics`` (MSE, MAE, mean
per-sample cosine similarity) is one dt_pair_stats launch over the two prediction batches (:11-85).

``analyze_noise_prediction`` is the reference's driver (:197-321): same signature, console lines, return dict and
``noise_metrics_size_{sf}.txt``.  Where the reference loops over its 10 timesteps (noise, two forwards, three
``.item()`` reductions each), every timestep here is one row group of a single batch: one dt_q_sample launch noises all
10 x B rows, one forward per model runs them all (the time-bias row of a group is shared by its B rows, tb_div = B) and
one dt_pair_stats launch reduces them.  The driver draws no figures (``visualize_noise_predictions`` and
``plot_noise_metrics_by_timestep`` are out of scope); loading a dataset is left to the config.

``noise_prediction_sweep`` is the capability the reference could only sample at 10 points: teacher-vs-student (and each
model-vs-true-noise) agreement at every timestep for many students, the teacher's forward shared by all of them.
"""
import os

import numpy as np
import torch

from ... import engine
from ..._hip import COND_NONE

# rows (timestep groups x images) per launch of the sweep: bounds the noised batch, the predictions and the forward workspace
SWEEP_CHUNK_ROWS = 512
N_TIMESTEPS = 10          # timesteps of the reference driver (:235)


def generate_noise_samples(batch_size, channels, image_size, device):
    """reference :11-24 (CPU generator draw, then moved to ``device``)."""
    return torch.randn(batch_size, channels, image_size, image_size).to(device)


def predict_noise(model, noisy_images, timesteps, device):
    """reference :26-41: eps = model(noisy_images, timesteps) in eval mode."""
    model.eval()
    with torch.no_grad():
        return model(noisy_images, timesteps)


def calculate_noise_metrics(teacher_noise, student_noise):
    """{'mse', 'mae', 'cosine_similarity'} as python floats (reference :43-85)."""
    if teacher_noise.shape != student_noise.shape:
        print(f"  Resizing student noise from {student_noise.shape} to {teacher_noise.shape}")
        student_noise = engine.resize_bilinear(student_noise, (teacher_noise.shape[2], teacher_noise.shape[3]))
    if not teacher_noise.is_cuda:
        from ..metrics.trajectory_metrics import _metrics_device
        dev = _metrics_device()
        teacher_noise, student_noise = teacher_noise.to(dev), student_noise.to(dev)
    B = teacher_noise.shape[0]
    X = teacher_noise.detach().float().reshape(1, B, -1).contiguous()
    Y = student_noise.detach().float().reshape(1, B, -1).contiguous()
    E = X.shape[2]
    f32 = np.float32
    st = engine.device_pair_stats(X, Y)[:, 0].cpu().numpy()                  # [B,5] float64
    mse = float(f32(st[:, 0].sum()) / f32(B * E))
    mae = float(f32(st[:, 1].sum()) / f32(B * E))
    eps = f32(1e-12)                                                          # F.normalize's clamp
    nx = np.maximum(np.sqrt(st[:, 3].astype(f32)), eps)
    ny = np.maximum(np.sqrt(st[:, 4].astype(f32)), eps)
    cos = st[:, 2].astype(f32) / (nx * ny)
    return {"mse": mse, "mae": mae, "cosine_similarity": float(np.mean(cos, dtype=f32))}


# ---------------------------------------------------------------------- the driver and the sweep
def _alpha_bars(config, t_max):
    """Python-float alpha_bar_t for t = 0 .. t_max: the reference's running product (:246-250); a prefix of the product
    of t is the product of t - 1, so one pass gives every t with the same operations in the same order."""
    out, ab = [], 1.0
    for i in range(t_max + 1):
        beta_i = config.beta_start + (config.beta_end - config.beta_start) * i / config.timesteps
        alpha_i = 1.0 - beta_i
        ab *= alpha_i
        out.append(ab)
    return out


def noise_coefficients(config, t_list):
    """fp32 host tensor [len(t_list), 2] of (sqrt(ab_t), sqrt(1 - ab_t)) (:253-268): the python float rounded to fp32 (what
    ``torch.as_tensor`` does), ``1 - ab`` in fp32, then the IEEE (correctly rounded) fp32 square root.  That is the value
    torch.sqrt gives on the host the reference vectors were taken on; torch's CPU sqrt is not correctly rounded on every
    x86 host (1 ulp off for some t on others), so numpy's IEEE sqrt keeps the coefficients the same on every host."""
    t_list = [int(t) for t in t_list]
    if not t_list:
        return torch.empty(0, 2)
    abs_ = _alpha_bars(config, max(t_list))
    ab = np.array([abs_[t] for t in t_list], dtype=np.float64).astype(np.float32)
    return torch.from_numpy(np.stack([np.sqrt(ab), np.sqrt(np.float32(1) - ab)], axis=1).astype(np.float32))


def _eps(model, x, t_list):
    """eps [n, B, C, H, W] of x [n, B, C, H, W]: one forward over every row, row group i at timestep t_list[i]."""
    n, B = x.shape[:2]
    h = engine.UNetHandle.for_module(model)
    tb = h.time_bias(t_list, [COND_NONE] * n)
    return h.forward(x.reshape(n * B, *x.shape[2:]), tb, 1, B).reshape(x.shape)


def _per_t_metrics(st, E, true_noise=False):
    """Per-timestep {'mse', 'mae', 'cosine_similarity'} from dt_pair_stats sums st [B, n, 5] (host float64), with the
    arithmetic of ``calculate_noise_metrics``."""
    B, n = st.shape[:2]
    f32 = np.float32
    eps = f32(1e-12)                                                          # F.normalize's clamp
    out = []
    for i in range(n):
        s = np.ascontiguousarray(st[:, i])
        nx = np.maximum(np.sqrt(s[:, 3].astype(f32)), eps)
        ny = np.maximum(np.sqrt(s[:, 4].astype(f32)), eps)
        cos = s[:, 2].astype(f32) / (nx * ny)
        out.append({"mse": float(f32(s[:, 0].sum()) / f32(B * E)), "mae": float(f32(s[:, 1].sum()) / f32(B * E)),
                    "cosine_similarity": float(np.mean(cos, dtype=f32))})
    return out


def _true_mse(st, E):
    B = st.shape[0]
    f32 = np.float32
    return [float(f32(np.ascontiguousarray(st[:, i, 0]).sum()) / f32(B * E)) for i in range(st.shape[1])]


def _noise_prediction_metrics(teacher, students, images, t_list, noise, config=None, true_noise=False, teacher_eps=None):
    """The noise-prediction metrics of explicit inputs, everything on the device.

    ``images`` [B, C, H, W]; ``t_list`` n python ints; ``noise`` [n, B, C, H, W] (or a list of n [B, C, H, W]); ``students``
    one model or a mapping key -> model.  Launches: one dt_q_sample over all n x B rows, one forward of the teacher (or
    ``teacher_eps`` when the caller already has it), then per student one forward and one dt_pair_stats (two more with
    ``true_noise``: each model's eps against the drawn noise).

    Returns (metrics, noised [n, B, C, H, W], teacher eps [n, B, C, H, W]); metrics is a list (per t, in t_list order) of
    {'mse', 'mae', 'cosine_similarity'[, 'teacher_true_mse', 'student_true_mse']}, or a mapping key -> such a list.
    """
    from ...config import Config
    config = config if config is not None else Config()
    single = not isinstance(students, dict)
    models = {None: students} if single else students
    device = next(teacher.parameters()).device
    images = images.to(device).float().contiguous()
    z = torch.stack(list(noise)) if isinstance(noise, (list, tuple)) else noise
    z = z.to(device).float().contiguous()
    n, B = z.shape[:2]
    E = images[0].numel()
    t_list = [int(t) for t in t_list]
    with torch.cuda.device(device):
        coef = noise_coefficients(config, t_list).pin_memory().to(device, non_blocking=True)
        x = engine.q_sample(images, z, coef)
        if teacher_eps is None:
            teacher_eps = _eps(teacher, x, t_list)
        X = teacher_eps.reshape(n, B, E)
        Z = z.reshape(n, B, E)
        parts = {}
        t_true = engine.device_pair_stats(X, Z) if true_noise else None
        for key, m in models.items():
            Y = _eps(m, x, t_list).reshape(n, B, E)
            parts[key] = [engine.device_pair_stats(X, Y)] + ([engine.device_pair_stats(Y, Z)] if true_noise else [])
        host = torch.stack([p for ps in parts.values() for p in ps] + ([t_true] if true_noise else [])).cpu().numpy()
    out, k = {}, 0
    for key, ps in parts.items():
        per_t = _per_t_metrics(host[k], E)
        if true_noise:
            for d, tm, sm in zip(per_t, _true_mse(host[-1], E), _true_mse(host[k + 1], E)):
                d["teacher_true_mse"], d["student_true_mse"] = tm, sm
        out[key] = per_t
        k += len(ps)
    return (out[None] if single else out), x, teacher_eps


def _dataset_images(config, device):
    """One shuffled batch of 10 test images (:228-232); the config must provide the dataset."""
    if not hasattr(config, "get_test_dataset"):
        raise ValueError("analyze_noise_prediction: the config has no get_test_dataset(); pass fixed_samples "
                         "(a [B, C, H, W] image tensor) instead")
    from torch.utils.data import DataLoader
    images, _ = next(iter(DataLoader(config.get_test_dataset(), batch_size=10, shuffle=True)))
    return images.to(device)


def format_noise_metrics(results):
    """The text of noise_metrics_size_{sf}.txt (:303-313)."""
    lines = [f"Average MSE: {results['avg_mse']:.6f}\n", f"Average MAE: {results['avg_mae']:.6f}\n",
             f"Average Cosine Similarity: {results['avg_cosine_similarity']:.6f}\n\n", "Metrics by Timestep:\n"]
    for t, metrics in sorted(results["metrics_by_timestep"].items()):
        lines += [f"  Timestep {t}:\n", f"    MSE: {metrics['mse']:.6f}\n", f"    MAE: {metrics['mae']:.6f}\n",
                  f"    Cosine Similarity: {metrics['cosine_similarity']:.6f}\n"]
    return "".join(lines)


def analyze_noise_prediction(teacher_model, student_model, config, output_dir=None, size_factor=None, fixed_samples=None):
    """Reference :197-321 on the device (see the module docstring); returns {'avg_mse', 'avg_mae', 'avg_cosine_similarity',
    'metrics_by_timestep': {t: {'mse', 'mae', 'cosine_similarity'}}} and writes noise_metrics_size_{sf}.txt.

    The noise is drawn as the reference draws it -- one ``torch.randn_like(images)`` per timestep, in timestep order, on
    the images' device -- all before the first launch; the forwards use no RNG, so the generator ends where the
    reference's would."""
    if output_dir is None:
        output_dir = os.path.join(config.analysis_dir, "noise_prediction", f"size_{size_factor}")
    os.makedirs(output_dir, exist_ok=True)
    print(f"Analyzing noise prediction for size factor {size_factor}...")
    device = next(teacher_model.parameters()).device
    teacher_model.eval()
    student_model.eval()
    if fixed_samples is not None:
        print(f"Using {len(fixed_samples)} fixed samples for consistent comparison")
        images = fixed_samples.to(device)
    else:
        images = _dataset_images(config, device)
    t_list = torch.linspace(0, config.timesteps - 1, N_TIMESTEPS, dtype=torch.long).tolist()
    noise = [torch.randn_like(images) for _ in t_list]
    per_t, _, _ = _noise_prediction_metrics(teacher_model, student_model, images, t_list, noise, config)
    metrics_by_timestep = {}
    for t, metrics in zip(t_list, per_t):
        metrics_by_timestep[t] = metrics
    avg_mse = np.mean([metrics['mse'] for metrics in metrics_by_timestep.values()])
    avg_mae = np.mean([metrics['mae'] for metrics in metrics_by_timestep.values()])
    avg_cosine = np.mean([metrics['cosine_similarity'] for metrics in metrics_by_timestep.values()])
    results = {"avg_mse": avg_mse, "avg_mae": avg_mae, "avg_cosine_similarity": avg_cosine,
               "metrics_by_timestep": metrics_by_timestep}
    with open(os.path.join(output_dir, f"noise_metrics_size_{size_factor}.txt"), "w") as f:
        f.write(format_noise_metrics(results))
    print(f"  Average MSE: {avg_mse:.6f}")
    print(f"  Average MAE: {avg_mae:.6f}")
    print(f"  Average Cosine Similarity: {avg_cosine:.6f}")
    return results


def noise_prediction_sweep(teacher_model, student_models, images, timesteps=None, seed=None, true_noise_metrics=True,
                           config=None):
    """Teacher-vs-student noise-prediction agreement at many timesteps for many students:
    ``{sf: {t: {'mse', 'mae', 'cosine_similarity'[, 'teacher_true_mse', 'student_true_mse']}}}``.

    ``student_models`` maps a size factor to a model; ``timesteps`` None means every t in 0 .. T-1 (T = config.timesteps,
    ``config`` None: the default ``Config()``).  The per-t noise is one ``randn`` of the images' shape per timestep, in
    timestep order, on the images' device: from the global generator (as ``analyze_noise_prediction`` draws it) or, with
    ``seed``, from a private ``torch.Generator`` seeded with it.  ``*_true_mse`` is each model's eps-MSE against the drawn
    noise (the per-t training loss).

    Rows are processed in chunks of max(1, SWEEP_CHUNK_ROWS // B) = max(1, 512 // B) timesteps: per chunk one dt_q_sample,
    ONE teacher forward shared by every student, then per student one forward and its dt_pair_stats.  A student's chunking
    and launches do not depend on which other students are in the call, so neither do its values."""
    from ...config import Config
    config = config if config is not None else Config()
    t_list = list(range(config.timesteps)) if timesteps is None else [int(t) for t in timesteps]
    device = next(teacher_model.parameters()).device
    teacher_model.eval()
    for m in student_models.values():
        m.eval()
    images = images.to(device).float().contiguous()
    B = images.shape[0]
    gen = None if seed is None else torch.Generator(device=device).manual_seed(int(seed))
    per_chunk = max(1, SWEEP_CHUNK_ROWS // B)
    out = {sf: {} for sf in student_models}
    for c0 in range(0, len(t_list), per_chunk):
        ts = t_list[c0:c0 + per_chunk]
        noise = [torch.randn_like(images) if gen is None else torch.randn(images.shape, generator=gen, device=device)
                 for _ in ts]
        res, _, _ = _noise_prediction_metrics(teacher_model, dict(student_models), images, ts, noise, config,
                                              true_noise=true_noise_metrics)
        for sf, per_t in res.items():
            for t, metrics in zip(ts, per_t):
                out[sf][t] = metrics
    return out
