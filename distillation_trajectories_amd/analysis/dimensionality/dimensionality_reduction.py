"""Joint teacher/student PCA and t-SNE of trajectories (reference analysis/dimensionality/dimensionality_reduction.py,
its second and effective ``dimensionality_reduction_analysis``), fitted on the device by TrajectoryPCA and TrajectoryTSNE.

Same directories, item handling, console lines and return value as the reference.  Instead of the figures, each
trajectory directory receives ``pca_trajectory.npz`` (teacher and student score rows, explained_variance_ratio) and, for
pairs of at most 500 rows, ``tsne_trajectory.npz`` (teacher and student embedding rows, kl_divergence).
UMAP is not run: ``umap`` is no dependency of this package.
"""
import os

import numpy as np
import torch

from .pca import TrajectoryPCA
from .tsne import TrajectoryTSNE

MAX_TRAJECTORIES = 3     # the reference stops after 3 trajectories "to avoid excessive computation"
MAX_TSNE_ROWS = 500      # the reference skips t-SNE for larger pairs


def flat_rows(trajectory):
    """fp32 [n, E] tensor of a trajectory's states: ``item[0]`` of each item (an (x, t) tuple, or a [1, C, H, W] tensor),
    flattened, as the reference's ``[item[0] for item in traj]`` then ``img.flatten()``; device tensors stay there."""
    rows = [item[0] if isinstance(item[0], torch.Tensor) else torch.as_tensor(np.asarray(item[0])) for item in trajectory]
    dev = next((r.device for r in rows if r.is_cuda), rows[0].device)
    return torch.stack([r.detach().reshape(-1).float().to(dev) for r in rows])


def joint_pca(teacher_traj, student_traj, n_components):
    """(teacher scores, student scores, explained_variance_ratio) numpy, of the PCA fitted on the stacked rows."""
    t_rows, s_rows = flat_rows(teacher_traj), flat_rows(student_traj)
    dev = t_rows.device if t_rows.is_cuda else s_rows.device
    combined = torch.cat([t_rows.to(dev), s_rows.to(dev)])
    pca = TrajectoryPCA(n_components=n_components)
    result = pca.fit_transform(combined)
    result = result.cpu().numpy() if isinstance(result, torch.Tensor) else result
    return result[: len(t_rows)], result[len(t_rows):], pca.explained_variance_ratio_


def joint_tsne(teacher_traj, student_traj):
    """(teacher embedding, student embedding, kl_divergence) numpy, of the t-SNE fitted on the stacked rows with the
    reference's arguments: perplexity min(30, n // 5), random_state 42."""
    t_rows, s_rows = flat_rows(teacher_traj), flat_rows(student_traj)
    dev = t_rows.device if t_rows.is_cuda else s_rows.device
    combined = torch.cat([t_rows.to(dev), s_rows.to(dev)])
    tsne = TrajectoryTSNE(n_components=2, perplexity=min(30, combined.shape[0] // 5), random_state=42)
    result = tsne.fit_transform(combined)
    result = result.cpu().numpy() if isinstance(result, torch.Tensor) else result
    return result[: len(t_rows)], result[len(t_rows):], tsne.kl_divergence_


def dimensionality_reduction_analysis(teacher_trajectories, student_trajectories, config, output_dir=None,
                                      size_factor=None):
    """Joint 2-component PCA and t-SNE of at most 3 teacher/student trajectory pairs; returns the absolute output directory.
    ``output_dir`` is ignored, as in the reference: the directory is config.dimensionality_dir[/size_{sf}]."""
    output_dir = config.dimensionality_dir
    if size_factor is not None:
        output_dir = os.path.join(output_dir, f"size_{size_factor}")
    os.makedirs(output_dir, exist_ok=True)

    print(f"Performing dimensionality reduction analysis for size factor {size_factor}...")

    for traj_idx, (teacher_traj, student_traj) in enumerate(zip(teacher_trajectories, student_trajectories)):
        if traj_idx >= MAX_TRAJECTORIES:
            break
        traj_dir = os.path.join(output_dir, f"trajectory_{traj_idx}")
        os.makedirs(traj_dir, exist_ok=True)

        print(f"  Performing PCA for trajectory {traj_idx}...")
        try:
            teacher_pca, student_pca, ratio = joint_pca(teacher_traj, student_traj, 2)
            np.savez(os.path.join(traj_dir, "pca_trajectory.npz"), teacher=teacher_pca, student=student_pca,
                     explained_variance_ratio=ratio)
        except Exception as e:
            print(f"  Error performing PCA: {e}")

        if len(teacher_traj) + len(student_traj) <= MAX_TSNE_ROWS:
            print(f"  Performing t-SNE for trajectory {traj_idx}...")
            try:
                teacher_tsne, student_tsne, kl = joint_tsne(teacher_traj, student_traj)
                np.savez(os.path.join(traj_dir, "tsne_trajectory.npz"), teacher=teacher_tsne, student=student_tsne,
                         kl_divergence=kl)
            except Exception as e:
                print(f"  Error performing t-SNE: {e}")
        else:
            print(f"  Skipping t-SNE for trajectory {traj_idx} (too many points)")

        print(f"  Skipping UMAP for trajectory {traj_idx} (not run here)")

    print(f"Dimensionality reduction analysis completed for size factor {size_factor}")
    return os.path.abspath(output_dir)
