"""Dimensionality analysis of teacher and student trajectories (reference analysis/dimensionality/): the exact PCA
and the exact t-SNE run on the device (pca.py, tsne.py); UMAP is not run."""
from .dimensionality_reduction import dimensionality_reduction_analysis
from .latent_space import generate_latent_space_visualization
