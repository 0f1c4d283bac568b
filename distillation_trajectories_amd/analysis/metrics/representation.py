"""What the networks represent, block by block: linear centered kernel alignment (CKA, Kornblith et al. 2019) between the
eight residual-block outputs of two U-Nets on the same inputs, with the debiased estimator of Nguyen, Raghu and Kornblith
(2021) beside it -- the plain estimator is biased towards 1 when the samples are few against the feature width, which a
block output of 128 x 16 x 16 features always is.  The Grams are n x n, so the channel counts of the two models need not
agree.  Activations never leave the device (engine.device_cka: csrc/dt_cka.hip); only the 8 x 8 score tables do."""
import os

import numpy as np
import torch

from ... import engine
from ..._hip import COND_ONE

BLOCKS = engine.BLOCK_NAMES


def _block_grams(model, x, tb, tb_div):
    """Grams of the eight block outputs of one forward of ``model`` on x, formed before the workspace is reused"""
    handle = engine.UNetHandle.for_module(model)
    return engine.device_cka_gram(handle.block_features(x, tb, 1, tb_div))


def _time_bias(model, x, t, cond):
    return engine.time_bias_rows(engine.UNetHandle.for_module(model), x.shape[0], t, cond)


def _check_n(n):
    if not engine.CKA_MIN_N <= n <= engine.CKA_MAX_N:
        raise ValueError(f"CKA needs {engine.CKA_MIN_N} <= samples <= {engine.CKA_MAX_N}, got {n}")


def cka_layers(model_a, model_b, x, t, cond=None):
    """CKA between every block of ``model_a`` and every block of ``model_b`` on the same x [n, C, H, W] at timestep(s)
    ``t`` (``cond`` as the models take it; None: the unconditional pass).  Returns numpy ``cka`` and ``cka_unbiased``
    [8, 8] (row: block of a, column: block of b), ``status_a`` and ``status_b`` [8] (engine.CKA_* bits) and ``blocks``."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("x must be a tensor [n, C, H, W]")
    _check_n(x.shape[0])
    device = next(model_a.parameters()).device
    with torch.cuda.device(device):
        x = x.to(device)
        ga = _block_grams(model_a, x, *_time_bias(model_a, x, t, cond))
        gb = _block_grams(model_b, x, *_time_bias(model_b, x, t, cond))
        r = engine.device_cka(ga, gb)
        return {"cka": r["cka"].cpu().numpy(), "cka_unbiased": r["cka_unbiased"].cpu().numpy(),
                "status_a": r["status_a"].cpu().numpy(), "status_b": r["status_b"].cpu().numpy(), "blocks": list(BLOCKS)}


def cka_sweep(teacher_model, student_models, config, num_samples, guidance_scale=None, every=1, output_dir=None):
    """Layer-wise CKA of every student with one teacher along the teacher's trajectories.  The trajectories come from
    ``sample_grid`` as ``pca_sweep`` and ``lpips_sweep`` run it (``noise_table(42, ...)``, sample s from seed 42 + s) at
    ``guidance_scale``.  Of the T states that are the input of a forward, every ``every``-th plus the last is taken
    (``perceptual.state_indices``); at each, the teacher and every student are forwarded on the TEACHER's states at that
    timestep with the condition on (the conditional pass of the reference's distillation loss).  The teacher's Grams are
    formed once per state and scored against themselves and against every student's.

    Returns numpy ``cka`` and ``cka_unbiased`` [n_students][n_states][8][8] (row: teacher block, column: student block),
    ``teacher_self`` and ``teacher_self_unbiased`` [n_states][8][8], ``status`` [1 + n_students][n_states][8] (teacher
    first), ``states``, ``timesteps`` and ``blocks``, and writes one ``cka_student_{k}.npz`` per student under
    ``output_dir`` (default ``config.analysis_dir``/cka).  ValueError, before anything is sampled, for fewer than 4 or more
    than 2048 samples, and for a model that declares a resolution (an ``image_size`` attribute) other than the
    config's.  The project's U-Nets are convolutional and declare none: for them the resolution is ``config.image_size``
    alone, and every model runs at it."""
    from ..trajectory_engine import sample_grid
    from ...synthetic import noise_table
    from .perceptual import state_indices
    students = list(student_models)
    if not students:
        raise ValueError("cka_sweep needs at least one student")
    if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)):
        raise ValueError(f"num_samples={num_samples!r} must be an int")
    _check_n(num_samples)
    C, H, T, S = config.channels, config.image_size, config.timesteps, int(num_samples)
    for m in [teacher_model] + students:
        if getattr(m, "image_size", H) != H:
            raise ValueError("cka_sweep forwards every model on the teacher's states: every model needs the teacher's resolution")
    idx = state_indices(T, every)
    timesteps = [T - 1 - i for i in idx]
    device = next(teacher_model.parameters()).device
    if output_dir is None:
        output_dir = os.path.join(config.analysis_dir, "cka")
    os.makedirs(output_dir, exist_ok=True)
    for m in [teacher_model] + students:
        m.eval()
    keys = ("cka", "cka_unbiased")
    with torch.cuda.device(device):
        table = noise_table(42, S + T - 1, (1, C, H, H)).reshape(S + T - 1, -1).to(device)
        th = engine.UNetHandle.for_module(teacher_model)
        states = sample_grid(th, table, 0, S, T, [guidance_scale], H, H)[guidance_scale]
        own = {k: [] for k in keys}
        cross = [{k: [] for k in keys} for _ in students]
        status = [[] for _ in range(1 + len(students))]
        for i, t in zip(idx, timesteps):
            x = states[i].reshape(S, C, H, H).contiguous()
            tb_of = lambda m: engine.UNetHandle.for_module(m).time_bias([t], [COND_ONE])
            gt = _block_grams(teacher_model, x, tb_of(teacher_model), S)
            r = engine.device_cka(gt)
            for k in keys:
                own[k].append(r[k])
            status[0].append(gt.status)
            for j, m in enumerate(students):
                gs = _block_grams(m, x, tb_of(m), S)
                r = engine.device_cka(gt, gs)
                for k in keys:
                    cross[j][k].append(r[k])
                status[1 + j].append(gs.status)
        host = lambda rows: torch.stack(rows).cpu().numpy()
        res = {"cka": np.stack([host(c["cka"]) for c in cross]),
               "cka_unbiased": np.stack([host(c["cka_unbiased"]) for c in cross]),
               "teacher_self": host(own["cka"]), "teacher_self_unbiased": host(own["cka_unbiased"]),
               "status": np.stack([host(s) for s in status]), "states": np.array(idx), "timesteps": np.array(timesteps),
               "blocks": np.array(BLOCKS)}
    for j in range(len(students)):
        np.savez(os.path.join(output_dir, f"cka_student_{j}.npz"), cka=res["cka"][j], cka_unbiased=res["cka_unbiased"][j],
                 teacher_self=res["teacher_self"], teacher_self_unbiased=res["teacher_self_unbiased"],
                 status=res["status"][[0, 1 + j]], states=res["states"], timesteps=res["timesteps"], blocks=res["blocks"])
    return res
