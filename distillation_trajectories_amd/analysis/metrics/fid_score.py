"""FID-input sampling and the FID formula (reference analysis/metrics/fid_score.py:61-93, 199-318).

The reference's fourth sampler (``p_sample_loop(model, x, config)``, :261-318) is the textbook DDPM posterior
with beta_t = beta_start + (beta_end-beta_start)*t/T and a running-product alpha_bar; its step
``x = (x - c0*eps)/sqrt(alpha_t) [+ sqrt(beta_t)*z]`` has exactly the shape of the fused update kernel's
MANAGER rule, so it runs device-resident with per-step coefficients computed on the host the way the
reference computes them (python floats -> fp32 0-dim tensors).  ``generate_samples`` batches all samples into
one loop (the reference runs them one by one); noise is drawn from the CPU generator in the reference's
order.  ``calculate_fid`` is the reference's numpy/scipy formula.

The InceptionV3 features (reference :19-56) run on the device (``inception.InceptionHandle``, include/dt_hip_inception.h)
with the user's copy of torchvision's pretrained weights (``weights=`` or ``DT_INCEPTION_WEIGHTS``; never downloaded).
``calculate_and_visualize_fid`` is the reference's driver (:96-198) without the figure.

``stats="device"`` (or ``DT_FID_STATS=device``) keeps the features on the device and takes the Fréchet distance there
too (``calculate_fid_device``, ``engine.device_fid_auto``): one double comes back.  With at most 2048 samples in the
smaller set that is the sample-space route (``engine.device_fid``, include/dt_hip_fid.h); with more in both sets, as FID is
normally reported, the feature-space route (``engine.device_fid_cov``, include/dt_hip_fid_cov.h).  The default,
``"host"``, is the reference's numpy/scipy formula on the copied features.  ``fid_sweep`` scores several students against
one teacher in one batched device call.
"""
import os

import numpy as np
import torch
from scipy import linalg

from ... import engine
from ... import inception
from ..._hip import COND_NONE, RULE_MANAGER


def calculate_fid(features_1, features_2):
    """Fréchet distance between two feature sets (reference :61-93), 999.0 placeholder below 2 samples."""
    if len(features_1) < 2 or len(features_2) < 2:
        print("  Warning: Not enough samples for a proper FID calculation.")
        print(f"  Number of samples in set 1: {len(features_1)}")
        print(f"  Number of samples in set 2: {len(features_2)}")
        print("  Returning a placeholder FID score of 999.0")
        return 999.0
    mu1, sigma1 = features_1.mean(axis=0), np.cov(features_1, rowvar=False)
    mu2, sigma2 = features_2.mean(axis=0), np.cov(features_2, rowvar=False)
    ssdiff = np.sum((mu1 - mu2) ** 2.0)
    covmean = linalg.sqrtm(sigma1.dot(sigma2))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return ssdiff + np.trace(sigma1 + sigma2 - 2.0 * covmean)


def stats_mode(stats=None):
    """"host" or "device": ``stats`` if given, else ``$DT_FID_STATS``, else "host"."""
    mode = stats if stats is not None else (os.environ.get("DT_FID_STATS") or "host")
    if mode not in ("host", "device"):
        raise ValueError(f"stats (or DT_FID_STATS) must be 'host' or 'device', got {mode!r}")
    return mode


def calculate_fid_device(features_1, features_2):
    """``calculate_fid`` with the arithmetic on the device, in fp64 (``engine.device_fid_auto``): fp32 features [N, D] that
    are on the device already, or host tensors / arrays that are uploaded first; returns a Python float.  The same 999.0
    placeholder below 2 samples.  Up to 2048 samples in the smaller set go the sample-space route, longer sets (up to
    131072 samples each, D <= 2048) the feature-space one (``engine.fid_route``); NaN if a feature is NaN or infinite."""
    if len(features_1) < 2 or len(features_2) < 2:
        print("  Warning: Not enough samples for a proper FID calculation.")
        print(f"  Number of samples in set 1: {len(features_1)}")
        print(f"  Number of samples in set 2: {len(features_2)}")
        print("  Returning a placeholder FID score of 999.0")
        return 999.0
    sets = [torch.as_tensor(f) for f in (features_1, features_2)]
    device = next((t.device for t in sets if t.is_cuda), torch.device("cuda"))
    sets = [t if t.is_cuda else t.to(device) for t in sets]
    return float(engine.device_fid_auto(sets[0], sets[1])["fid"][0])


def posterior_coefficients(config):
    """[(c0, sqrt(alpha_t), sqrt(beta_t))] for t = T-1..0 with the reference's arithmetic (:284-305)."""
    T = config.timesteps
    rows = []
    for t in range(T - 1, -1, -1):
        beta_t = config.beta_start + (config.beta_end - config.beta_start) * t / T
        alpha_t = 1.0 - beta_t
        alpha_bar_t = 1.0
        for i in range(t + 1):
            alpha_bar_t *= 1.0 - (config.beta_start + (config.beta_end - config.beta_start) * i / T)
        b, a, ab = torch.as_tensor(beta_t), torch.as_tensor(alpha_t), torch.as_tensor(alpha_bar_t)
        rows.append((float((1 - a) / torch.sqrt(1 - ab)), float(torch.sqrt(a)), float(torch.sqrt(b))))
    return rows


def noise_kw(noise):
    """The ``noise`` keyword for a callee only when the caller was given one, so that a call without it is the call it was."""
    return {} if noise is None else {"noise": noise}


def _run(model, x0, config, z):
    """Final samples [S,C,H,W] (device) for start images x0[S,C,H,W] and step noise z[T-1,S,E]."""
    h = engine.UNetHandle.for_module(model)
    S, C, H, W = x0.shape
    E, T = C * H * W, config.timesteps
    device = next(model.parameters()).device
    traj = torch.empty(T + 1, S, E, dtype=torch.float32, device=device)
    traj[0].copy_(x0.reshape(S, E))
    order = list(range(T - 1, -1, -1))
    tb = h.time_bias(order, [COND_NONE] * T)
    h.sample(RULE_MANAGER, traj, H, W, tb, 1, posterior_coefficients(config), [t > 0 for t in order],
             z=None if z is None else z.reshape(-1, E).to(device), z_shift=[k * S for k in range(T)])
    return traj[T].reshape(S, C, H, W).clone()


def p_sample_loop(model, x, config, noise=None):
    """Reference :261-318: denoise ``x`` through all config.timesteps steps; returns the final sample.  ``noise``: "host" (the
    default, unless ``$DT_NOISE`` says otherwise) draws the step noise on the CPU generator, "device" makes the same draws on
    the device and leaves the generator where the host draws would have (``engine.noise_mode``)."""
    model.eval()
    T = config.timesteps
    if engine.noise_mode(noise) == "device":
        z = None
        if T > 1:           # one stream continued from the host generator: T - 1 draws of x.numel() elements
            z = torch.empty(T - 1, x.shape[0], x[0].numel(), dtype=torch.float32, device=next(model.parameters()).device)
            engine.device_randn(state=engine.HostGenerator(), draws=T - 1, E=x.numel(), out=z, device=z.device)
        return _run(model, x.detach().float(), config, z)
    zs = [torch.randn(x.shape) for _ in range(T - 1)]            # one CPU-generator draw per step with t > 0
    z = torch.stack(zs).reshape(T - 1, x.shape[0], -1) if zs else None
    return _run(model, x.detach().float(), config, z)


def generate_samples(model, config, num_samples, device, fixed_samples=None, noise=None):
    """Reference :199-259: ``num_samples`` final samples [N,C,H,W]; all of them advance in one batched loop.  ``noise`` as for
    ``p_sample_loop``: with "device" the start and step draws of all samples are one stream continued from the host
    generator's state, written straight into the step-major buffers the sampler reads."""
    model.eval()
    image_size = getattr(model, "image_size", config.image_size)
    T = config.timesteps
    device_noise = engine.noise_mode(noise) == "device"
    starts, zs = [], []
    if fixed_samples is not None:
        print(f"    Using {min(num_samples, len(fixed_samples))} fixed samples as starting points")
        n = len(fixed_samples[:num_samples])
    else:
        n = num_samples
    if device_noise and fixed_samples is None:
        # the reference's draw order is sample-major (start of sample i, then its T - 1 steps): draw i * T + k goes to row
        # i of step k, so buf[0] holds the starts and buf[1:] the step noise
        E = config.channels * image_size * image_size
        buf = torch.empty(T, n, E, dtype=torch.float32, device=next(model.parameters()).device)
        if n:
            engine.device_randn(state=engine.HostGenerator(), draws=(n, T), E=E, out=buf, strides=(0, E, n * E),
                                device=buf.device)
        return _run(model, buf[0].reshape(n, config.channels, image_size, image_size), config, buf[1:] if T > 1 else None)
    for i in range(n):           # reference draw order: start noise of sample i, then its T-1 step draws
        if fixed_samples is not None:
            x = fixed_samples[i:i + 1].clone().cpu().float()
            if x.shape[2] != image_size or x.shape[3] != image_size:
                x = engine.resize_bilinear(x, (image_size, image_size)).cpu()
        else:
            x = torch.randn(1, config.channels, image_size, image_size)
        starts.append(x)
        if not device_noise:
            zs.append(torch.stack([torch.randn(x.shape) for _ in range(T - 1)]) if T > 1 else None)
    x0 = torch.cat(starts)
    if device_noise:             # fixed starting points: only the T - 1 step draws per sample
        z = None
        if T > 1:
            E = x0[0].numel()
            z = torch.empty(T - 1, n, E, dtype=torch.float32, device=next(model.parameters()).device)
            engine.device_randn(state=engine.HostGenerator(), draws=(n, T - 1), E=E, out=z, strides=(0, E, n * E),
                                device=z.device)
        return _run(model, x0, config, z)
    z = torch.stack(zs, dim=1).reshape(T - 1, n, -1) if T > 1 else None
    return _run(model, x0, config, z)


class InceptionModel:
    """Reference :19-56: ``get_features(images)`` -> [N, 2048] numpy features of images in [-1, 1] (mapped by
    (x + 1) / 2, resized to 299 x 299 and normalised with ImageNet's mean / std), in batches of 32 as the reference
    runs them.  ``weights`` is a path or a state dict of torchvision's Inception3 (default: ``$DT_INCEPTION_WEIGHTS``)."""

    def __init__(self, device, weights=None):
        self.device = torch.device(device)
        self.handle = inception.InceptionHandle(inception.read_weights(weights), self.device)

    def get_features(self, images):
        return extract_features(images, self, batch_size=32, in_scale=0.5, in_shift=0.5).cpu().numpy()


def extract_features(images, model=None, weights=None, device=None, batch_size=64, in_scale=1.0, in_shift=0.0):
    """[N, 2048] fp32 features on the device for images [N, 3, H, W] (1 <= H, W <= 299), ``batch_size`` images per
    launch sequence.  ``in_scale * x + in_shift`` is applied first: (0.5, 0.5) is get_features' (x + 1) / 2, the default
    (1, 0) takes the images as given (compute_fid).  An image's features do not depend on the batching.  ``model`` is
    an InceptionModel; without one, one is built on ``device`` (default cuda) from ``weights``."""
    inception.check_images(images)
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if model is None:
        model = InceptionModel(device if device is not None else (images.device if images.is_cuda else "cuda"), weights)
    h = model.handle
    out = torch.empty(len(images), inception.N_FEATURES, dtype=torch.float32, device=h.device)
    for i in range(0, len(images), batch_size):
        h.features(images[i:i + batch_size], in_scale, in_shift, out=out[i:i + batch_size])
    return out


def calculate_and_visualize_fid(teacher_model, student_model, config, output_dir=None, size_factor=None,
                                fixed_samples=None, weights=None, stats=None, noise=None):
    """Reference :96-198: FID between teacher and student samples; console lines, ``fid_score_size_{sf}.txt`` and the
    returned ``{"fid_score": ...}`` as the reference's.  No figure is drawn.  ``stats``: "host" (the default, unless
    ``$DT_FID_STATS`` says otherwise) or "device" (``stats_mode``); ``noise`` as for ``generate_samples``."""
    mode = stats_mode(stats)
    if output_dir is None:
        output_dir = os.path.join(config.analysis_dir, "fid", f"size_{size_factor}")
    os.makedirs(output_dir, exist_ok=True)
    print(f"Calculating FID scores for size factor {size_factor}...")
    device = next(teacher_model.parameters()).device
    teacher_model.eval()
    student_model.eval()
    num_samples = config.num_samples if hasattr(config, 'num_samples') else 50
    print("  Generating samples from teacher model...")
    teacher_samples = generate_samples(teacher_model, config, num_samples, device, fixed_samples=fixed_samples, **noise_kw(noise))
    print("  Generating samples from student model...")
    student_samples = generate_samples(student_model, config, num_samples, device, fixed_samples=fixed_samples, **noise_kw(noise))
    print("  Extracting features using InceptionV3...")
    inception_model = InceptionModel(device, weights)
    if mode == "device":
        teacher_features = extract_features(teacher_samples, inception_model, batch_size=32, in_scale=0.5, in_shift=0.5)
        student_features = extract_features(student_samples, inception_model, batch_size=32, in_scale=0.5, in_shift=0.5)
    else:
        teacher_features = inception_model.get_features(teacher_samples)
        student_features = inception_model.get_features(student_samples)
    print("  Calculating FID score...")
    fid_score = (calculate_fid_device if mode == "device" else calculate_fid)(teacher_features, student_features)
    print(f"  FID score for size factor {size_factor}: {fid_score:.4f}")
    with open(os.path.join(output_dir, f"fid_score_size_{size_factor}.txt"), "w") as f:
        f.write(f"FID Score: {fid_score:.4f}\n")
    return {"fid_score": fid_score}


def fid_sweep(teacher_model, student_models, config, num_samples, weights=None, fixed_samples=None, noise=None):
    """FID of every student against one teacher: the teacher's samples and features once, each student's samples and
    features (``generate_samples`` in that order, so the CPU generator is consumed as by one
    ``calculate_and_visualize_fid`` call for the teacher followed by the students), then one batched
    ``engine.device_fid_auto`` with the teacher's features shared.  Returns numpy ``fid [n_students]`` and
    ``parts [n_students, 4]`` (float64) and ``status [n_students]``; nothing else leaves the device.  ``noise`` as for
    ``generate_samples``."""
    student_models = list(student_models)
    if not student_models:
        raise ValueError("fid_sweep needs at least one student model")
    if num_samples < 2:
        raise ValueError(f"fid_sweep needs num_samples >= 2, got {num_samples}")
    device = next(teacher_model.parameters()).device
    inception_model = InceptionModel(device, weights)

    def features(model):
        model.eval()
        samples = generate_samples(model, config, num_samples, device, fixed_samples=fixed_samples, **noise_kw(noise))
        return extract_features(samples, inception_model, batch_size=32, in_scale=0.5, in_shift=0.5)

    teacher = features(teacher_model)
    students = torch.stack([features(m) for m in student_models])
    res = engine.device_fid_auto(teacher, students)
    return {k: v.cpu().numpy() for k, v in res.items()}
