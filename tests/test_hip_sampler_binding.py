"""Which C entry each of the handle's five public methods reaches, and with which scalar arguments.

``forward``, ``forward_mixed``, ``sample``, ``sample_mixed`` and ``sample_masked`` share one private forward and one private
sampler in engine.py; this pins what they hand to the library.  The handle's ``lib`` is wrapped in a recorder that notes, for
the five batch entries, the entry's name and its B, n_pass, B_single, tb_div, n_steps and w_scalar (those it takes).  EXPECTED
was taken by running ``record()`` below, unchanged, on the commit before the methods were folded together: a call of a shape
the handle has not run yet is preceded by one forward of that shape, which settles its launch plan; a second call is not."""
import pytest
import torch

from distillation_trajectories_amd import engine
from distillation_trajectories_amd._hip import COND_NONE, COND_ONE, COND_ZERO, RULE_ENGINE, RULE_PSAMPLE

pytestmark = pytest.mark.gpu

E = 3 * 16 * 16
# positions of the scalar arguments in each entry's argument list (include/dt_hip.h, include/dt_hip_edit.h)
ENTRIES = {
    "dt_unet_forward": dict(B=2, n_pass=3, tb_div=7),
    "dt_unet_forward_mixed": dict(B=2, B_single=3, tb_div=7),
    "dt_sample_trajectory": dict(B=2, n_pass=3, n_steps=6, w_scalar=14),
    "dt_sample_trajectory_mixed": dict(B=2, B_single=3, n_steps=6, tb_div=8),
    "dt_sample_trajectory_masked": dict(B=2, n_pass=3, B_single=4, n_steps=7, tb_div=9, w_scalar=16),
}


class Recorder:
    """the library, with the calls of the batch entries noted in ``calls``"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ENTRIES:
            return fn

        def call(*args):
            self.calls.append((name, {k: getattr(args[i], "value", args[i]) for k, i in ENTRIES[name].items()}))
            return fn(*args)
        return call


def record(engine_module, state_dict, device):
    """[(label, [(entry, scalars)])] of the table of calls, on a fresh handle"""
    h = engine_module.UNetHandle(state_dict, device)
    h.lib = rec = Recorder(h.lib)
    g = torch.Generator().manual_seed(3)
    ts = [20, 0]
    coef, noise, shift = [(0.99, 0.05, 0.02), (0.97, 0.06, 0.0)], [True, False], [0, 4]
    z = torch.randn(8, E, generator=g).to(device)
    w4, w3 = torch.tensor([0.0, 0.0, 3.0, 5.0]).to(device), torch.tensor([0.0, 3.0, 5.0]).to(device)
    mask = (torch.rand(1, E, generator=g) > 0.5).float().to(device)
    known = torch.randn(4, E, generator=g).to(device)

    def traj(B, n_steps=2):
        t = torch.zeros(n_steps + 1, B, E, device=device)
        t[0] = torch.randn(B, E, generator=g).to(device)
        return t

    def tb(step):
        return h.time_bias([t for t in ts for _ in step], step * len(ts))
    tb1, tb2 = tb([COND_NONE]), tb([COND_ZERO, COND_ONE])
    tb_m2, tb_m1 = tb([COND_NONE, COND_ZERO, COND_ONE]), tb([COND_NONE] + [COND_ZERO] * 2 + [COND_ONE] * 2)
    mrow = torch.zeros(4, dtype=torch.int32, device=device)
    table = [
        ("sample, two passes, a shape not run yet",
         lambda: h.sample(RULE_PSAMPLE, traj(3), 16, 16, tb2, 2, coef, noise, z=z, z_shift=shift)),
        ("sample, two passes, again",
         lambda: h.sample(RULE_PSAMPLE, traj(3), 16, 16, tb2, 2, coef, noise, z=z, z_shift=shift)),
        ("sample, one pass, w_scalar 3",
         lambda: h.sample(RULE_ENGINE, traj(3), 16, 16, tb1, 1, coef, noise, z=z, w_scalar=3.0)),
        ("sample, no steps, a shape not run yet",
         lambda: h.sample(RULE_ENGINE, traj(4, 0), 16, 16, tb2, 2, [], [])),
        ("sample_mixed, B 4, b_single 2, tb_div 2, a shape not run yet",
         lambda: h.sample_mixed(RULE_PSAMPLE, traj(4), 16, 16, tb_m2, 2, 2, coef, noise, z, None, shift, w4)),
        ("sample_mixed, again",
         lambda: h.sample_mixed(RULE_PSAMPLE, traj(4), 16, 16, tb_m2, 2, 2, coef, noise, z, None, shift, w4)),
        ("sample_masked, defaults, a shape not run yet",
         lambda: h.sample_masked(RULE_ENGINE, traj(4), 16, 16, tb1, 1, coef, noise, mask, known, mask_row=mrow, z=z)),
        ("sample_masked, b_single 2, tb_div 2",
         lambda: h.sample_masked(RULE_PSAMPLE, traj(4), 16, 16, tb_m2, 2, coef, noise, mask, known, mask_row=mrow, z=z, w=w4, b_single=2,
                                 tb_div=2)),
        ("sample_masked, b_single 1, tb_div 1, a shape not run yet",
         lambda: h.sample_masked(RULE_PSAMPLE, traj(3), 16, 16, tb_m1, 2, coef, noise, mask, known, mask_row=mrow[:3], z=z, w=w3,
                                 b_single=1, tb_div=1)),
        ("sample_masked, b_single 0, tb_div None, two passes, w_scalar 2",
         lambda: h.sample_masked(RULE_PSAMPLE, traj(3), 16, 16, tb2, 2, coef, noise, mask, known, mask_row=mrow[:3], z=z, w_scalar=2.0,
                                 b_single=0, tb_div=None)),
        ("forward, one pass", lambda: h.forward(traj(3)[0].reshape(3, 3, 16, 16), tb1[:1], 1, 3)),
        ("forward, two passes, tb_div 1",
         lambda: h.forward(traj(2)[0].reshape(2, 3, 16, 16), tb([COND_ZERO] * 2 + [COND_ONE] * 2)[:4], 2, 1)),
        ("forward_mixed, B 4, b_single 2, tb_div 2", lambda: h.forward_mixed(traj(4)[0].reshape(4, 3, 16, 16), tb_m2[:3], 2, 2)),
    ]
    out = []
    for label, call in table:
        del rec.calls[:]
        call()
        out.append((label, list(rec.calls)))
    torch.cuda.synchronize()
    return out


EXPECTED = [('sample, two passes, a shape not run yet',
  [('dt_unet_forward', {'B': 3, 'n_pass': 2, 'tb_div': 3}), ('dt_sample_trajectory', {'B': 3, 'n_pass': 2, 'n_steps': 2, 'w_scalar': 1.0})]),
 ('sample, two passes, again', [('dt_sample_trajectory', {'B': 3, 'n_pass': 2, 'n_steps': 2, 'w_scalar': 1.0})]),
 ('sample, one pass, w_scalar 3',
  [('dt_unet_forward', {'B': 3, 'n_pass': 1, 'tb_div': 3}), ('dt_sample_trajectory', {'B': 3, 'n_pass': 1, 'n_steps': 2, 'w_scalar': 3.0})]),
 ('sample, no steps, a shape not run yet', [('dt_sample_trajectory', {'B': 4, 'n_pass': 2, 'n_steps': 0, 'w_scalar': 1.0})]),
 ('sample_mixed, B 4, b_single 2, tb_div 2, a shape not run yet',
  [('dt_unet_forward_mixed', {'B': 4, 'B_single': 2, 'tb_div': 2}),
   ('dt_sample_trajectory_mixed', {'B': 4, 'B_single': 2, 'n_steps': 2, 'tb_div': 2})]),
 ('sample_mixed, again', [('dt_sample_trajectory_mixed', {'B': 4, 'B_single': 2, 'n_steps': 2, 'tb_div': 2})]),
 ('sample_masked, defaults, a shape not run yet',
  [('dt_unet_forward', {'B': 4, 'n_pass': 1, 'tb_div': 4}),
   ('dt_sample_trajectory_masked', {'B': 4, 'B_single': 0, 'n_pass': 1, 'n_steps': 2, 'tb_div': 4, 'w_scalar': 1.0})]),
 ('sample_masked, b_single 2, tb_div 2',
  [('dt_sample_trajectory_masked', {'B': 4, 'B_single': 2, 'n_pass': 2, 'n_steps': 2, 'tb_div': 2, 'w_scalar': 1.0})]),
 ('sample_masked, b_single 1, tb_div 1, a shape not run yet',
  [('dt_unet_forward_mixed', {'B': 3, 'B_single': 1, 'tb_div': 1}),
   ('dt_sample_trajectory_masked', {'B': 3, 'B_single': 1, 'n_pass': 2, 'n_steps': 2, 'tb_div': 1, 'w_scalar': 1.0})]),
 ('sample_masked, b_single 0, tb_div None, two passes, w_scalar 2',
  [('dt_sample_trajectory_masked', {'B': 3, 'B_single': 0, 'n_pass': 2, 'n_steps': 2, 'tb_div': 3, 'w_scalar': 2.0})]),
 ('forward, one pass', [('dt_unet_forward', {'B': 3, 'n_pass': 1, 'tb_div': 3})]),
 ('forward, two passes, tb_div 1', [('dt_unet_forward', {'B': 2, 'n_pass': 2, 'tb_div': 1})]),
 ('forward_mixed, B 4, b_single 2, tb_div 2', [('dt_unet_forward_mixed', {'B': 4, 'B_single': 2, 'tb_div': 2})])]


def test_public_methods_reach_the_entries_they_reached_before(models):
    dev = torch.device("cuda:0")
    sd = {k: v.float() for k, v in models(0.25).state_dict().items() if v.dtype.is_floating_point}
    got = record(engine, sd, dev)
    for (label, calls), (want_label, want) in zip(got, EXPECTED):
        assert label == want_label and calls == want, (label, calls, want)
    assert len(got) == len(EXPECTED)
