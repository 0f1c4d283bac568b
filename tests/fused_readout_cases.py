"""The models, images and batch layouts of the block-by-block check of the fused small-model kernel (tests/fused_readout.py):
chosen on the CPU -- tests/test_fused_readout_host.py asserts that the float64 reference alone is not degenerate on them -- and
run unchanged on the device by tests/test_hip_fused_blocks.py."""
import functools
from typing import NamedTuple

import torch

import fused_readout as fr
from fused_readout import COND_NONE, COND_ONE, COND_ZERO, Layout


class Model(NamedTuple):
    sf: float
    C: int
    dims: tuple        # real (c0, c1)
    padded: tuple      # what the fused kernel pads them to: its layer table depends on these alone
    x_seed: int


# one model per padded-dims class (the k-split of the low levels differs between c1p = 32, 48 and 64), odd real channel
# counts where the size sweep has them; one and two image channels on the class with the most padding
MODELS = {
    "sf0.1_16/32": Model(0.1, 3, (16, 32), (16, 32), 301),
    "sf0.15_19/38": Model(0.15, 3, (19, 38), (32, 48), 302),
    "sf0.2_25/50": Model(0.2, 3, (25, 50), (32, 64), 303),
    "sf0.25_32/64": Model(0.25, 3, (32, 64), (32, 64), 304),
    "sf0.15_19/38_C1": Model(0.15, 1, (19, 38), (32, 48), 305),
    "sf0.15_19/38_C2": Model(0.15, 2, (19, 38), (32, 48), 306),
}

# the smallest batches with a half-empty last workgroup (two rows a workgroup), both passes of a CFG pair, and a mixed batch
# whose pass boundary falls inside a workgroup; every time-bias row differs from its neighbours
LAYOUTS = {lay.name: lay for lay in (
    Layout("one_pass_B3", 3, 1, 0, 1, ((7, COND_NONE), (23, COND_ONE), (41, COND_ZERO))),
    Layout("cfg_B4", 4, 2, 0, 4, ((9, COND_NONE), (9, COND_ONE))),
    Layout("mixed_B3_single1", 3, 2, 1, 1, ((3, COND_NONE), (11, COND_ZERO), (27, COND_ZERO), (11, COND_ONE), (27, COND_ONE))),
    # the layouts of test_hip_fused.py::test_fused_cfg_pair_and_mixed_batch_rows
    Layout("cfg_B6", 6, 2, 0, 6, ((7, COND_NONE), (7, COND_ONE))),
    Layout("mixed_B6_single2", 6, 2, 2, 2, ((3, COND_NONE), (3, COND_ZERO), (3, COND_ZERO), (3, COND_ONE), (3, COND_ONE))),
)}
SWEEP_LAYOUTS = ("one_pass_B3", "cfg_B4", "mixed_B3_single1")
ROW_LAYOUTS = ("cfg_B6", "mixed_B6_single2")
ROW_MODEL, ROW_BLOCKS = "sf0.2_25/50", (3, 4)        # the 2x2 and 1x1 levels: two rows share one MFMA tile
LOOP_MODEL, LOOP_BLOCKS = "sf0.2_25/50", (4, 7)
BLOCK_IDS = (-1, 0, 1, 2, 3, 4, 5, 6, 7)


@functools.lru_cache(maxsize=None)
def state_dict(model):
    """fp32 weights of a case's model: the seeded synthetic model of its size factor (synthetic.make_model)"""
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model
    m = MODELS[model]
    cfg = Config()
    cfg.image_size, cfg.channels = 16, m.C
    state = torch.get_rng_state()
    sd = {k: v.detach().clone().float() for k, v in make_model(DiffusionUNet, cfg, m.sf).state_dict().items()
          if v.dtype.is_floating_point}
    torch.set_rng_state(state)
    assert (sd["enc1.conv2.weight"].shape[0], sd["enc2.conv2.weight"].shape[0]) == m.dims
    return sd


@functools.lru_cache(maxsize=None)
def inputs(model, layout):
    """fused_readout.Inputs of a (model, layout): the image batch and, computed once and shared, the block outputs of the
    unchanged model in fp32 and float64"""
    m, lay = MODELS[model], LAYOUTS[layout]
    x = torch.randn(lay.B, m.C, 16, 16, generator=torch.Generator().manual_seed(m.x_seed))
    return fr.make_inputs(state_dict(model), lay, x)


def references(model, layout, r):
    return fr.references(inputs(model, layout), r)
