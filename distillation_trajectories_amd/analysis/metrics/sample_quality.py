"""Set-level sample quality beside FID, on the device: KID (the unbiased MMD^2 with the cubic polynomial kernel), improved
precision / recall (Kynkäänniemi et al. 2019) and density / coverage (Naeem et al. 2020) of a teacher's and a student's
Inception features (``engine.device_quality``, include/dt_hip_quality.h, which holds the definitions).  The first set is
always the "real" one (the teacher), the second the "generated" one (a student).  Sets of up to 2048 rows go through whole
Gram matrices, longer ones (up to 131072 rows each, k <= 1023) through row panels (``engine.device_quality_stream``,
include/dt_hip_quality_stream.h); ``engine.device_quality_auto`` chooses, and FID beside them goes through
``engine.device_fid_auto``.

FID is strongly biased at the sample counts used here (50 by default, 64 - 512 in the grids); KID is not.  FID also folds
fidelity and diversity into one number, which guidance scale and student size trade against each other; precision and
density measure the first, recall and coverage the second.

``kid_subset_tables`` makes the subset tables of the usual "mean and deviation over subsets" form of KID on the host (no
device RNG); ``quality_sweep`` scores several students against one teacher beside ``fid_sweep``'s FID, and
``guidance_quality_sweep`` does so per guidance scale on the final states of the grid's sampler."""
import numpy as np
import torch

from ... import engine
from . import fid_score


def kid_subset_tables(n_a, n_b, num_subsets, subset_size, seed=0):
    """Two int32 tables [num_subsets, subset_size] of row numbers, into a set of n_a and one of n_b rows.  The recipe,
    so that anyone can reproduce a table: with ``rs = np.random.RandomState(seed)``, for s = 0, 1, ... in turn,
    ``idx_a[s] = rs.permutation(n_a)[:subset_size]`` and then ``idx_b[s] = rs.permutation(n_b)[:subset_size]``."""
    if num_subsets < 1:
        raise ValueError(f"num_subsets must be >= 1, got {num_subsets}")
    if not 2 <= subset_size <= min(n_a, n_b):
        raise ValueError(f"subset_size must be in [2, min(n_a, n_b)] = [2, {min(n_a, n_b)}], got {subset_size}")
    rs = np.random.RandomState(seed)
    idx_a = np.empty((num_subsets, subset_size), np.int32)
    idx_b = np.empty((num_subsets, subset_size), np.int32)
    for s in range(num_subsets):
        idx_a[s] = rs.permutation(n_a)[:subset_size]
        idx_b[s] = rs.permutation(n_b)[:subset_size]
    return idx_a, idx_b


def _on_device(features_1, features_2):
    sets = [torch.as_tensor(f) for f in (features_1, features_2)]
    device = next((t.device for t in sets if t.is_cuda), torch.device("cuda"))
    return [t if t.is_cuda else t.to(device) for t in sets]


def _subsets(n_a, n_b, num_subsets, subset_size, seed):
    if not num_subsets:
        return None
    return kid_subset_tables(n_a, n_b, num_subsets, min(n_a, n_b) if subset_size is None else subset_size, seed)


def calculate_kid_device(features_1, features_2, num_subsets=0, subset_size=None, seed=0):
    """KID between two feature sets [N, D] (fp32, on the device already, or host tensors / arrays that are uploaded
    first), in fp64 on the device: {"kid": the full-set unbiased estimate, "kid_mean", "kid_std": mean and population
    standard deviation over ``num_subsets`` subsets of ``subset_size`` rows (``kid_subset_tables`` with ``seed``; default
    size min(N1, N2)), NaN when ``num_subsets`` is 0}, Python floats.  Up to 131072 rows per set; with more than 2048 rows in
    a set a subset takes at most 2048 rows (the usual protocol is 100 subsets of 1000), so ``subset_size`` must be given."""
    a, b = _on_device(features_1, features_2)
    r = engine.device_quality_auto(a, b, k=1, subsets=_subsets(len(a), len(b), num_subsets, subset_size, seed))
    sub = r["kid_subsets"][0].cpu().numpy()
    return {"kid": float(r["kid"][0]), "kid_mean": float(sub.mean()) if len(sub) else float("nan"),
            "kid_std": float(sub.std()) if len(sub) else float("nan")}


def calculate_prdc_device(features_1, features_2, k=5):
    """{"precision", "recall", "density", "coverage"} (Python floats) of the generated set features_2 against the real
    set features_1, with the k-th nearest-neighbour radii of ``prdc`` (self included, strict ``<``).  Up to 131072 rows per
    set; k <= 1023 when a set has more than 2048 rows."""
    a, b = _on_device(features_1, features_2)
    r = engine.device_quality_auto(a, b, k=k)
    return {name: float(r[name][0]) for name in ("precision", "recall", "density", "coverage")}


_SCORES = ("kid", "kid_subsets", "precision", "recall", "density", "coverage", "counts", "status")


def quality_sweep(teacher_model, student_models, config, num_samples, weights=None, fixed_samples=None, k=5,
                  num_subsets=0, subset_size=None, seed=0, noise=None):
    """FID, KID, precision / recall and density / coverage of every student against one teacher.  Samples and features
    are made exactly as ``fid_sweep`` makes them (same sampler, same consumption of the CPU generator: its ``fid`` comes
    out bit for bit under the same seed); then one batched ``engine.device_fid_auto`` and one batched
    ``engine.device_quality_auto`` with the teacher's features shared (up to 2048 samples: the calls ``engine.device_fid`` and
    ``engine.device_quality`` as before; up to 131072: the feature-space and row-panel routes, subsets of at most 2048
    rows).  Returns numpy arrays per student: ``fid``, ``kid`` [n], ``kid_subsets`` [n, num_subsets], ``precision``,
    ``recall``, ``density``, ``coverage`` [n], ``counts`` [n, 4], ``status`` [n] (that of the quality call; 1: a non-finite
    feature).  ``noise``: where the sampler's noise is drawn, as for ``fid_score.generate_samples``."""
    student_models = list(student_models)
    if not student_models:
        raise ValueError("quality_sweep needs at least one student model")
    if num_samples < 2:
        raise ValueError(f"quality_sweep needs num_samples >= 2, got {num_samples}")
    device = next(teacher_model.parameters()).device
    inception_model = fid_score.InceptionModel(device, weights)

    def features(model):
        model.eval()
        samples = fid_score.generate_samples(model, config, num_samples, device, fixed_samples=fixed_samples,
                                             **fid_score.noise_kw(noise))
        return fid_score.extract_features(samples, inception_model, batch_size=32, in_scale=0.5, in_shift=0.5)

    teacher = features(teacher_model)
    students = torch.stack([features(m) for m in student_models])
    n_a, n_b = teacher.shape[0], students.shape[1]
    fid = engine.device_fid_auto(teacher, students)
    res = engine.device_quality_auto(teacher, students, k=k, subsets=_subsets(n_a, n_b, num_subsets, subset_size, seed))
    out = {name: res[name].cpu().numpy() for name in _SCORES}
    out["fid"] = fid["fid"].cpu().numpy()
    return out


def guidance_quality_sweep(teacher_model, student_models, config, guidance_scales, num_samples, weights=None, k=5,
                           num_subsets=0, subset_size=None, seed=0, noise=None):
    """The same scores per guidance scale: ``sample_grid`` for each model exactly as ``lpips_sweep`` and ``pca_sweep`` run
    it (sample s starts from seed 42 + s, one noise table), Inception features of the final states with the map
    (0.5, 0.5), and per scale one batched ``engine.device_fid_auto`` and ``engine.device_quality_auto`` of every student
    against the teacher at that scale (the limits of ``quality_sweep``).  Returns numpy arrays [n_students][n_scales]
    (``kid_subsets`` [..., num_subsets], ``counts`` [..., 4]).  ``noise``: where the noise table is made
    (``synthetic.noise_table``)."""
    from ..trajectory_engine import sample_grid
    from ...synthetic import noise_table
    C, H, T, S = config.channels, config.image_size, config.timesteps, num_samples
    students, scales = list(student_models), list(guidance_scales)
    if not students:
        raise ValueError("guidance_quality_sweep needs at least one student model")
    if S < 2:
        raise ValueError(f"guidance_quality_sweep needs num_samples >= 2, got {S}")
    device = next(teacher_model.parameters()).device
    inception_model = fid_score.InceptionModel(device, weights)
    subsets = _subsets(S, S, num_subsets, subset_size, seed)

    def features(grid, gs):
        return fid_score.extract_features(grid[gs][T].reshape(S, C, H, H).contiguous(), inception_model, batch_size=32,
                                          in_scale=0.5, in_shift=0.5)

    with torch.cuda.device(device):
        table = noise_table(42, S + T - 1, (1, C, H, H), **fid_score.noise_kw(noise)).reshape(S + T - 1, -1).to(device)
        t_grid = sample_grid(engine.UNetHandle.for_module(teacher_model), table, 0, S, T, scales, H, H)
        s_grids = [sample_grid(engine.UNetHandle.for_module(m), table, 0, S, T, scales, H, H) for m in students]
        cols = []
        for gs in scales:
            teacher = features(t_grid, gs)
            batch = torch.stack([features(grid, gs) for grid in s_grids])
            res = engine.device_quality_auto(teacher, batch, k=k, subsets=subsets)
            col = {name: res[name] for name in _SCORES}
            col["fid"] = engine.device_fid_auto(teacher, batch)["fid"]
            cols.append(col)
        return {name: torch.stack([col[name] for col in cols], dim=1).cpu().numpy() for name in cols[0]}
