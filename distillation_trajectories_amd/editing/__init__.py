"""The reference's ``editing/`` stage on the HIP path: masked inpainting, latent manipulation, prompt editing (drop-ins for
the reference's modules of the same names) and the batched sweeps."""
from .sweep import inpainting_sweep, manipulation_sweep

__all__ = ["inpainting_sweep", "manipulation_sweep"]
