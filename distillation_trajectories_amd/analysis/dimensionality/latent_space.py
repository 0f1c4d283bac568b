"""3-component joint PCA of a teacher/student trajectory pair (reference analysis/dimensionality/latent_space.py),
fitted on the device by TrajectoryPCA.  Same directory, list-of-lists handling, console lines and return values as the
reference; instead of the figures the directory receives ``latent_space.npz`` (teacher and student score rows,
explained_variance_ratio)."""
import os

import numpy as np

from .dimensionality_reduction import joint_pca


def generate_latent_space_visualization(teacher_trajectory, student_trajectory, config, size_factor=None):
    """Returns the absolute output directory, or (after a printed error) the directory as configured."""
    output_dir = config.latent_space_dir
    if size_factor is not None:
        output_dir = os.path.join(output_dir, f"size_{size_factor}")
    os.makedirs(output_dir, exist_ok=True)

    print(f"Generating 3D latent space visualization for size factor {size_factor}...")

    # a list of trajectories: the first one is used
    if isinstance(teacher_trajectory, list) and isinstance(teacher_trajectory[0], list):
        teacher_traj = teacher_trajectory[0]
        student_traj = student_trajectory[0]
    else:
        teacher_traj = teacher_trajectory
        student_traj = student_trajectory

    try:
        teacher_pca, student_pca, ratio = joint_pca(teacher_traj, student_traj, 3)
        np.savez(os.path.join(output_dir, "latent_space.npz"), teacher=teacher_pca, student=student_pca,
                 explained_variance_ratio=ratio)
        print(f"Latent space visualization completed for size factor {size_factor}")
        return os.path.abspath(output_dir)
    except Exception as e:
        print(f"Error generating latent space visualization: {e}")
        return output_dir
