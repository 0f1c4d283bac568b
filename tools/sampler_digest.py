#!/usr/bin/env python3
"""SHA-256 of what the sampler's five public methods compute on a seeded synthetic model.  Two checkouts that print the same
lines compute the same bits through ``UNetHandle.forward``, ``forward_mixed``, ``sample``, ``sample_mixed`` and
``sample_masked``; nothing else of the handle is used, so ``--root DIR`` runs another checkout (one without the masked loop
prints no masked lines).

The model is the size-factor-0.25 synthetic model at 16 x 16, on the fused path and with the fused kernel off.  Per path:

  * ``forward`` with one and two passes at B = 3, ``forward_mixed`` at B = 3 / b_single = 1 / tb_div = 1 and at
    B = 4 / b_single = 2 / tb_div = 2: eps;
  * per rule (ENGINE, PSAMPLE, MANAGER) a loop of 3 steps, the last without noise, the step noise read through a ``z_row``
    table with a ``z_shift`` that is not the identity: ``sample`` with one and two passes, the guidance weight as a scalar
    and as a per-image vector, and ``sample_mixed`` at the two mixed shapes; then ``sample_masked`` in the same forms, the
    known rows read through a row table: the whole trajectory buffer;
  * a 4-step ``sample`` under ``DT_GRAPH=1`` on a side stream, called twice with the same buffers, so that the second call
    is a replay: the trajectory buffer after each call.

    python tools/sampler_digest.py [--root DIR]
"""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch   # noqa: E402

from distillation_trajectories_amd import engine   # noqa: E402
from distillation_trajectories_amd._hip import (COND_NONE, COND_ONE, COND_ZERO, RULE_ENGINE, RULE_MANAGER,   # noqa: E402
                                                 RULE_PSAMPLE)
from distillation_trajectories_amd.config import Config   # noqa: E402
from distillation_trajectories_amd.models import DiffusionUNet   # noqa: E402
from distillation_trajectories_amd.synthetic import make_model   # noqa: E402

DEV = torch.device("cuda:0")
E = 3 * 16 * 16
RULES = (("ENGINE", RULE_ENGINE), ("PSAMPLE", RULE_PSAMPLE), ("MANAGER", RULE_MANAGER))
TS = [30, 11, 0]                                     # the last step has no noise
COEF = [(0.99, 0.05, 0.02, 0.4), (0.98, 0.04, 0.03, 0.3), (0.97, 0.06, 0.0, 0.2)]
SHIFT = [4, 0, 9]
# (name, B, n_pass, b_single, tb_div or None for the plain entry's B, per-image weights)
FORMS = (("1 pass, scalar w", 3, 1, 0, None, False), ("1 pass, vector w", 3, 1, 0, None, True),
         ("2 passes, scalar w", 3, 2, 0, None, False), ("2 passes, vector w", 3, 2, 0, None, True),
         ("mixed B3 single1 div1", 3, 2, 1, 1, True), ("mixed B4 single2 div2", 4, 2, 2, 2, True))


def line(name, t):
    digest = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
    print(f"{name:64s} {digest}  finite {bool(torch.isfinite(t).all())}", flush=True)


def time_bias(h, ts, B, n_pass, b_single, tb_div):
    """the time-bias rows of a loop over ts: per step one row per pass, or the mixed batch's [single | pass 0 | pass 1]"""
    if b_single:
        step = [COND_NONE] * (b_single // tb_div) + [COND_ZERO] * ((B - b_single) // tb_div) + [COND_ONE] * ((B - b_single) // tb_div)
    else:
        step = [COND_ZERO, COND_ONE] if n_pass == 2 else [COND_NONE]
    return h.time_bias([t for t in ts for _ in step], step * len(ts))


def inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, E, generator=g).to(DEV)
    z = torch.randn(max(SHIFT) + B + 2, E, generator=g).to(DEV)
    z_row = torch.tensor([(2 * b + 1) % B for b in range(B)], dtype=torch.int32).to(DEV)
    w = torch.tensor([0.0, 2.5, 7.0, 4.0][:B]).to(DEV)
    known = (torch.rand(2, E, generator=g) * 2 - 1).to(DEV)
    mask = torch.zeros(1, 3, 16, 16)
    mask[:, :, 4:12, 3:13] = 1
    return x, z, z_row, w, known, mask.reshape(1, E).to(DEV)


def path_lines(h, path):
    for name, B, n_pass, b_single, tb_div, vector in FORMS:
        if vector and not b_single:
            continue          # (a forward has no guidance weight)
        x = inputs(B, 5)[0].reshape(B, 3, 16, 16)
        tb = time_bias(h, [17], B, n_pass, b_single, tb_div)
        eps = h.forward_mixed(x, tb, b_single, tb_div) if b_single else h.forward(x, tb, n_pass, B)
        line(f"{path} forward {name.replace(', scalar w', '')}", eps)
    for rule_name, rule in RULES:
        for masked in (False, True):
            if masked and not hasattr(h, "sample_masked"):
                continue
            for name, B, n_pass, b_single, tb_div, vector in FORMS:
                x, z, z_row, w, known, mask = inputs(B, 6)
                tb = time_bias(h, TS, B, n_pass, b_single, tb_div)
                traj = torch.zeros(len(TS) + 1, B, E, device=DEV)
                traj[0] = x
                noise = [t > 0 for t in TS]
                wv, ws = (w, 1.0) if vector else (None, 3.0)
                if masked:
                    mrow = torch.zeros(B, dtype=torch.int32, device=DEV)
                    krow = (torch.arange(B) % 2).to(torch.int32).to(DEV)
                    h.sample_masked(rule, traj, 16, 16, tb, n_pass, COEF, noise, mask, known, mrow, krow, z=z, z_row=z_row, z_shift=SHIFT,
                                    w=wv, w_scalar=ws, b_single=b_single, tb_div=tb_div)
                elif b_single:
                    h.sample_mixed(rule, traj, 16, 16, tb, tb_div, b_single, COEF, noise, z, z_row, SHIFT, w)
                else:
                    h.sample(rule, traj, 16, 16, tb, n_pass, COEF, noise, z=z, z_row=z_row, z_shift=SHIFT, w=wv, w_scalar=ws)
                line(f"{path} {rule_name} {'sample_masked' if masked else 'sample'} {name}", traj)


def replay_lines(h, path):
    B, ts = 3, [40, 30, 11, 0]
    x, z, z_row, _, _, _ = inputs(B, 7)
    tb = time_bias(h, ts, B, 2, 0, None)
    traj = torch.zeros(len(ts) + 1, B, E, device=DEV)
    traj[0] = x
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    os.environ["DT_GRAPH"] = "1"
    try:
        with torch.cuda.stream(side):
            for call in ("first call (capture)", "second call (replay)"):
                traj[1:].zero_()
                h.sample(RULE_PSAMPLE, traj, 16, 16, tb, 2, COEF + [(0.96, 0.02, 0.0, 0.1)], [t > 0 for t in ts], z=z, z_row=z_row,
                         z_shift=SHIFT + [1], w_scalar=3.0)
                line(f"{path} PSAMPLE sample 4 steps DT_GRAPH=1 {call}", traj)
        side.synchronize()
    finally:
        del os.environ["DT_GRAPH"]


def main():
    if not torch.cuda.is_available():
        sys.exit("sampler_digest.py runs on the GPU; none is visible")
    cfg = Config()
    cfg.image_size = 16
    sd = {k: v.float() for k, v in make_model(DiffusionUNet, cfg, 0.25).state_dict().items() if v.dtype.is_floating_point}
    for fused in (True, False):
        h = engine.UNetHandle(sd, DEV)
        h.set_fused(fused)
        assert h.fused_active(16, 16) == fused, h.dims
        path = "fused" if fused else "layered"
        path_lines(h, path)
        replay_lines(h, path)


if __name__ == "__main__":
    main()
