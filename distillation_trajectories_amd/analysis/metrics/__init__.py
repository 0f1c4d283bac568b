"""Set-level metrics of teacher and student samples (reference analysis/metrics/): FID (fid_score.py), LPIPS along the
trajectories (perceptual.py) and KID, precision / recall, density / coverage (sample_quality.py), all on the device."""
from .sample_quality import guidance_quality_sweep, quality_sweep
