#!/usr/bin/env python3
"""Launch-selection rules of the convolution hooks: tests/golden/launch_rules.{npz,json}.

Run on the GPU box from the repo root, with the library of the commit the records are taken from:
    python tests/golden/record_launch_rules.py SOURCE_COMMIT [OUT_PREFIX]
It only creates handles and calls the choice hooks (dt_unet_set_conv_choice, dt_unet_conv_choice, the plan table):
no convolution is launched.  tests/test_launch_rules.py recomputes the same records with the library under test.

  * grid: for each GRID_CASES (model, rows, H) and every (block, slot, bm, bn, splits, kind, fuse) of GRID_AXES, on a
    fresh plan (set_precision(AUTO)): the status of dt_unet_set_conv_choice, then dt_unet_conv_choice's report
    (bm, bn, splits, kind (+8 skip folded), tuned) of that slot and of the block's skip slot;
  * plans: engine.conv_choices() of every size factor at every SHAPES entry, untuned in each precision mode and with
    the committed plan table applied;
  * table: every entry of plans/gfx950.json is accepted and read back unchanged (checked here, not stored).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import ctypes          # noqa: E402
import numpy as np     # noqa: E402
import torch           # noqa: E402

from distillation_trajectories_amd import _hip, engine                 # noqa: E402
from distillation_trajectories_amd.config import Config               # noqa: E402
from distillation_trajectories_amd.models import DiffusionUNet        # noqa: E402
from distillation_trajectories_amd.synthetic import make_model        # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "launch_rules")
# read at handle creation / engine import (DT_NO_SHARED_ENC1, DT_PRECISION, DT_PLAN_TABLE) or by ensure_plan: the records
# are of the defaults
ENV = ("DT_AUTOTUNE", "DT_TUNE_CACHE", "DT_PRECISION", "DT_PLAN_TABLE", "DT_NO_SHARED_ENC1")
SIZES = (0.01, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0)
# (size factor, rows, H): sf 0.3 has odd channel-chunk counts; 4 rows of 64 x 64 is past the strip kernel's staging reach
GRID_CASES = ((1.0, 512, 16), (0.5, 512, 16), (0.3, 512, 16), (1.0, 4, 64))
GRID_AXES = dict(block=range(8), slot=range(3), bm=(64, 128, 256), bn=(64, 128), splits=range(1, 10), kind=range(6),
                 fuse=(0, 1))
# (rows, H, images, single-pass images): configs[0] (CFG off), [1], [2] (mixed), [3] (mixed, 8 scales per GPU), [4]
SHAPES = ((8, 16, 8, 0), (512, 16, 256, 0), (448, 16, 256, 64), (960, 16, 512, 64), (256, 32, 128, 0))
MODES = (("fp32", _hip.PREC_FP32), ("split-bf16", _hip.PREC_SPLIT_BF16), ("auto", _hip.PREC_AUTO))


def handle(sf):
    cfg = Config()
    cfg.image_size = 16
    return engine.UNetHandle(make_model(DiffusionUNet, cfg, sf).state_dict(), torch.device("cuda:0"))


def report(h, rows, H, imgs, single, block, slot):
    v = [ctypes.c_int() for _ in range(5)]
    _hip.check(h.lib.dt_unet_conv_choice(h.h, rows, H, H, imgs, single, block, slot, *map(ctypes.byref, v)), "dt_unet_conv_choice")
    return [x.value for x in v]


def choice_grid(h, rows, H):
    """status [8,3,3,2,9,6,2] and the two reports [..., 5] over GRID_AXES, for the two-pass shape of the rows"""
    split = (rows // 2, 0)
    axes = list(GRID_AXES.values())
    shape = tuple(len(a) for a in axes)
    status = np.zeros(shape, np.int16)
    slot_rep = np.zeros(shape + (5,), np.int16)
    skip_rep = np.zeros(shape + (5,), np.int16)
    for idx in np.ndindex(shape):
        block, slot, bm, bn, sp, kind, fuse = (a[i] for a, i in zip(axes, idx))
        _hip.check(h.lib.dt_unet_set_precision(h.h, _hip.PREC_AUTO), "dt_unet_set_precision")
        status[idx] = h.lib.dt_unet_set_conv_choice(h.h, rows, H, H, *split, block, slot, bm, bn, sp, kind, fuse)
        slot_rep[idx] = report(h, rows, H, *split, block, slot)
        skip_rep[idx] = report(h, rows, H, *split, block, 0)
    return status, slot_rep, skip_rep


def plan_reports(h):
    """{"<mode>|<rows>x<H>x<H>|<imgs>/<single>": conv_choices} untuned per mode, and "table|..." with the plan table"""
    out = {}
    for name, mode in MODES + (("table", _hip.PREC_AUTO),):
        h.set_precision(mode)
        for rows, H, imgs, single in SHAPES:
            h.ensure_plan(rows, H, H, imgs, single, tune=None if name == "table" else False)
            out[f"{name}|{rows}x{H}x{H}|{imgs}/{single}"] = [list(c) for c in h.conv_choices(rows, H, H)]
    h.set_precision(_hip.PREC_AUTO)
    return out


def table_mismatches(h, seen):
    """keys of plans/gfx950.json (for this handle's model) whose entries are refused or read back changed"""
    bad = []
    table = engine._Plans.table()
    for rows, H, imgs, single in SHAPES:
        key = h.plan_key(rows, H, H, imgs, single)
        if key not in table:
            continue
        seen.add(key)
        h.set_precision(_hip.PREC_AUTO)
        ok = all(h.lib.dt_unet_set_conv_choice(h.h, rows, H, H, imgs, single, *entry) == 0 for entry in table[key])
        if not ok or [list(c[:7]) for c in h._choices((rows, H, H, imgs, single))] != table[key]:
            bad.append(key)
    h.set_precision(_hip.PREC_AUTO)
    return bad


def main(source_commit, out=OUT):
    arrays, plans, seen, bad = {}, {}, set(), []
    handles = {sf: handle(sf) for sf in SIZES}
    for sf, rows, H in GRID_CASES:
        tag = f"sf{sf}_{rows}x{H}"
        arrays[f"status_{tag}"], arrays[f"slot_{tag}"], arrays[f"skip_{tag}"] = choice_grid(handles[sf], rows, H)
    for sf, h in handles.items():
        plans[str(sf)] = plan_reports(h)
        bad += table_mismatches(h, seen)
    assert not bad and seen == set(engine._Plans.table()), (bad, set(engine._Plans.table()) - seen)
    np.savez_compressed(out + ".npz", **arrays)
    meta = {"source_commit": source_commit, "made_by": "tests/golden/record_launch_rules.py",
            "grid_cases": GRID_CASES, "grid_axes": {k: list(v) for k, v in GRID_AXES.items()},
            "report": "[bm, bn, splits, kind + 8 * skip folded, tuned]", "shapes": SHAPES, "plans": plans}
    with open(out + ".json", "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True)
    print("wrote", out + ".{npz,json}", {k: int((v == 0).sum()) for k, v in arrays.items() if k.startswith("status")})


if __name__ == "__main__":
    assert not any(v in os.environ for v in ENV), ENV
    main(*sys.argv[1:3])
