"""Set-level metrics of teacher and student samples (reference analysis/metrics/): FID (fid_score.py), LPIPS along the
trajectories (perceptual.py) and KID, precision / recall, density / coverage (sample_quality.py), all on the device;
and, beyond the reference, the alignment of a teacher's and a student's trajectory in time (alignment.py) the
layer-wise CKA of what their blocks represent (representation.py), the spatial-frequency spectra of their states
(spectral.py), the sliced Wasserstein distance between their sets of states (sliced_wasserstein.py) and the Sinkhorn
divergence between those sets in the full state space (sinkhorn.py)."""
from .alignment import align_trajectories, alignment_pairs, alignment_sweep
from .representation import cka_layers, cka_sweep
from .sample_quality import guidance_quality_sweep, quality_sweep
from .sinkhorn import sinkhorn_pairs, sinkhorn_sweep, sinkhorn_trajectories
from .sliced_wasserstein import sliced_wasserstein_pairs, sliced_wasserstein_sweep, sliced_wasserstein_trajectories
from .spectral import spectral_pairs, spectral_sweep, spectral_trajectories
