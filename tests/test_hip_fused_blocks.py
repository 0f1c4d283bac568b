"""The fused small-model kernel (csrc/dt_fused.hip), one U-Net block at a time, against float64.

The kernel keeps every activation in LDS, so a block is read through weights (tests/fused_readout.py): in the readout model
M(j, k) the blocks 0 .. j keep their weights, everything downstream is transparent (exact copies, exact max pools, x2
bilinear upsamples) and the 0 / 1 head selects C channels of block j's output; over k every real channel is read.  For
every model of tests/fused_readout_cases.py (one per padded-dims class 16/32, 32/48, 32/64, odd real channel counts, 1 / 2 /
3 image channels), every j in -1 .. 7 (-1: every block transparent, eps is pools, selections and upsamples of the image) and
every batch layout (one pass B = 3 with a half-empty last workgroup, a CFG pair of B = 4, a mixed batch whose pass boundary
falls inside a workgroup; a time-bias row of its own per row or per pass) the fused forward of every M(j, k) is compared
per batch row with forward64 of the same M(j, k):

  * the worst row's relative L2 error over the row's concatenated readouts, and the worst row's max-abs error over the row's
    max-abs reference, each at most MARGIN = 4 x the larger of two yardsticks taken on the same M(j, k) and inputs: the fp32
    CPU oracle (oracle/unet_ref.py) and the layered device kernels (set_fused(False), PREC_FP32), whose own per-block error
    tests/test_hip_conv_blocks.py caps absolutely.  No constant is fixed in advance; neither yardstick is the code under test;
  * for j >= 0 the fused eps and the layered eps of the same M(j, k) differ by no more than the same bound;
  * j = -1: the values that reach the four corner pixels of eps (bilinear weights exactly 1 and 0) are bit-exact;
  * padding: what the non-carrier channels of the selecting blocks hold (input channel n % cin, or nothing at all) changes
    no value of eps, at the channel groups next to the padding boundary (channels 18 of 19, 24 of 25) and at group 0;
  * rows (j = 3, 4: the 2x2 and 1x1 levels, where two rows share an MFMA tile): the live row of a half-empty workgroup is
    bit-identical to the same image in a full workgroup; the CFG and mixed layouts of test_hip_fused.py meet the criterion
    row for row;
  * loop mode (j = 4, 7): one LOOP step with n_pass 1 and 2 equals forward + engine.cfg_update bit for bit on every M(j, k);
  * three further random models (tools/fuzz_fused.py's block mode, a short child process) meet the criterion.

tests/test_fused_readout_host.py proves without a GPU that the surgery is exact, that the inputs are not degenerate, and that
the criterion rejects a dropped border tap, swapped concat channels, a three-element pool window, a shifted time-bias row
and a K slice counted twice, each at its own block.

Measured on one MI355X (first run; the test prints the current figures with -s): errors against float64 in units of 1e-7,
[worst row's relative L2, worst row's max-abs over max-abs reference], the maximum over the batch layouts; K = readout models
(handles) of the block.  The largest ratio of a fused figure to the larger yardstick over all 166 (model, layout, block)
cells is 1.88 (sf 0.25, one pass, enc4, max-abs), of the 4 allowed; no cell needed an explanation from the code.

   j block        K    fused        layered      cpu fp32     fused - layered
  sf0.1_16/32
  -1 image        4    0.55 2.01    0.56 2.05    0.69 2.45    0.30 1.72
   0 enc1         6    0.95 2.16    0.91 2.30    1.00 3.00    0.53 1.49
   1 enc2        11    1.02 2.80    0.94 2.30    1.03 2.59    0.99 3.39
   2 enc3        11    0.99 3.06    0.87 2.80    1.00 2.40    1.07 2.84
   3 enc4        11    1.12 2.81    1.02 2.81    1.14 3.52    1.11 3.07
   4 bottleneck  11    1.18 2.73    1.13 2.73    1.38 4.52    1.48 2.49
   5 dec3        11    1.88 3.71    1.93 5.06    1.99 4.40    2.42 5.27
   6 dec2        11    1.89 3.42    1.73 2.64    1.90 3.27    2.13 4.05
   7 dec1         6    1.26 3.23    1.12 2.47    1.32 2.52    1.49 3.45
  sf0.15_19/38
  -1 image        4    0.60 1.78    0.58 1.96    0.66 2.07    0.35 1.94
   0 enc1         7    1.02 2.18    0.96 2.15    0.99 2.71    0.67 2.24
   1 enc2        13    1.59 3.58    1.43 2.69    1.46 2.86    1.43 3.05
   2 enc3        13    1.28 3.05    1.02 2.23    1.09 2.16    1.28 2.87
   3 enc4        13    1.29 3.00    1.03 3.18    1.12 2.83    1.40 3.21
   4 bottleneck  13    1.58 3.03    1.10 2.50    1.36 2.94    1.55 2.57
   5 dec3        13    1.73 3.33    1.83 4.67    1.97 4.01    2.30 5.45
   6 dec2        13    1.91 3.63    2.00 4.14    2.09 3.92    2.35 4.42
   7 dec1         7    1.91 3.46    1.62 3.57    1.68 3.18    2.11 4.58
  sf0.2_25/50
  -1 image        4    0.59 1.96    0.57 1.96    0.64 2.03    0.37 1.57
   0 enc1         9    0.96 2.41    0.89 2.41    0.87 2.16    0.69 1.86
   1 enc2        17    1.57 3.76    1.24 2.89    1.29 2.72    1.57 3.92
   2 enc3        17    1.30 3.44    0.98 2.81    1.06 2.67    1.34 3.49
   3 enc4        17    1.42 3.93    1.16 3.47    1.16 3.59    1.35 3.97
   4 bottleneck  17    1.70 3.74    1.34 3.00    1.53 3.94    1.81 3.53
   5 dec3        17    2.13 4.13    2.19 6.88    2.19 4.37    2.79 5.74
   6 dec2        17    1.83 3.44    1.71 3.41    1.81 3.82    2.12 4.83
   7 dec1         9    2.90 6.91    2.30 4.46    2.46 5.09    3.23 7.02
  sf0.25_32/64
  -1 image        4    0.62 2.28    0.62 2.28    0.68 2.44    0.35 1.63
   0 enc1        11    1.09 3.52    1.05 3.38    1.06 3.67    0.67 2.11
   1 enc2        22    1.65 3.72    1.30 3.11    1.41 3.19    1.62 4.08
   2 enc3        22    1.42 4.25    1.03 2.60    1.10 2.73    1.54 4.14
   3 enc4        22    1.43 4.89    1.02 3.04    1.05 2.66    1.44 4.84
   4 bottleneck  22    1.84 4.48    1.18 2.46    1.34 3.06    1.88 4.98
   5 dec3        22    2.38 4.30    2.32 4.98    2.38 4.99    3.06 5.72
   6 dec2        22    2.21 3.60    2.09 4.63    2.16 4.56    2.88 5.37
   7 dec1        11    2.54 5.76    2.02 4.02    2.08 4.72    2.84 6.38
  sf0.15_19/38_C1
  -1 image        4    0.65 2.06    0.66 2.06    0.70 2.16    0.35 1.63
   0 enc1        19    0.94 1.98    0.90 1.97    0.94 2.41    0.68 1.71
   1 enc2        38    1.33 3.54    1.13 2.96    1.24 2.65    1.26 2.97
   2 enc3        38    1.14 2.30    0.95 2.15    1.01 1.94    1.24 2.48
   3 enc4        38    1.10 2.89    1.05 2.59    1.12 2.71    1.19 2.98
   4 bottleneck  38    1.46 2.94    1.18 2.26    1.47 2.78    1.53 2.99
   5 dec3        38    1.72 3.29    2.26 4.66    2.10 4.85    2.61 4.76
   6 dec2        38    1.57 4.44    1.64 3.32    1.71 3.71    2.04 4.42
   7 dec1        19    1.99 3.63    1.59 3.66    1.75 3.62    2.17 3.39
  sf0.15_19/38_C2
  -1 image        4    0.68 1.94    0.68 1.94    0.66 2.34    0.44 2.17
   0 enc1        10    0.80 2.02    0.75 1.89    0.78 2.40    0.60 1.71
   1 enc2        19    1.21 3.10    1.05 2.86    1.18 2.87    1.21 3.01
   2 enc3        19    1.08 2.92    0.92 2.28    1.02 2.11    1.16 3.53
   3 enc4        19    1.23 2.99    1.01 2.43    1.10 2.59    1.18 3.42
   4 bottleneck  19    1.39 3.23    1.18 3.15    1.34 3.39    1.65 2.73
   5 dec3        19    1.86 3.39    2.57 4.76    2.00 4.47    2.77 4.25
   6 dec2        19    1.82 3.18    2.10 3.40    1.94 3.28    2.26 3.14
   7 dec1        10    2.49 4.14    2.11 3.45    2.30 4.20    2.93 5.20

Module time on that machine: 18.4 s for 64 items -- 15.5 s for the 63 in-process items (868 handles in the sweep; the slowest,
38 handles of the one-channel model, 0.64 s) and 2.9 s for the child process of the three random models.
"""
import time

import pytest
import torch
import torch.nn.functional as F

import fused_readout as fr
import fused_readout_cases as cases
from distillation_trajectories_amd import engine
from distillation_trajectories_amd._hip import COND_NONE, COND_ONE, RULE_PSAMPLE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWEEP = [cases.LAYOUTS[name] for name in cases.SWEEP_LAYOUTS]


@pytest.fixture(scope="module", autouse=True)
def cpu_threads():
    """float64 references on at most 16 threads (a GPU box may show many more cores than a job may use)"""
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(old, 16)))
    yield
    torch.set_num_threads(old)


@pytest.fixture(scope="module")
def table():
    """(model, layout, j) -> Measured, printed when the module is done: [worst row rel L2, worst row max-abs / max-abs]"""
    rows, t0 = {}, time.time()
    yield rows
    print(f"\nerrors against float64 [rel L2, max-abs], worst row; {len(rows)} (model, layout, block) cells; module time {time.time() - t0:.1f} s")
    for (model, layout, j), m in rows.items():
        print(f"  {model:16s} {layout:17s} j={j:2d} {(fr.BLOCKS[j] if j >= 0 else 'image'):10s} K={len(m.models):2d}: {m.line()}")
    for model in cases.MODELS:
        print(f"  maxima over layouts, {model}: fused / layered / cpu fp32 rel L2 by block: " + "  ".join(
            "/".join(f"{max(getattr(m, which)[0] for (mo, _, jj), m in rows.items() if mo == model and jj == j) * 1e7:.2f}"
                     for which in ("fused", "layered", "cpu")) for j in cases.BLOCK_IDS if any(mo == model and jj == j for mo, _, jj in rows))
              + "  [1e-7]")


def inputs_of(model, layouts):
    return {lay.name: cases.inputs(model, lay.name) for lay in layouts}


# ------------------------------------------------------------------ every block of every model
@pytest.mark.parametrize("j", cases.BLOCK_IDS)
@pytest.mark.parametrize("model", list(cases.MODELS))
def test_fused_block_against_float64(model, j, table):
    sd32 = cases.state_dict(model)
    got = fr.measure_block(sd32, j, SWEEP, inputs_of(model, SWEEP), DEV)
    failures = []
    for lay in SWEEP:
        m = got[lay.name]
        table[(model, lay.name, j)] = m
        print(f"\n  {model} {lay.name} j={j}: {m.line()}")
        width = fr.block_width(sd32, j)
        assert {c for r in m.models for c in r.chans} == set(range(width)) and m.eps["fused"].shape[1] == len(fr.row_images(lay))
        assert torch.isfinite(m.eps["fused"]).all()
        if not fr.within_margin(m.fused, [m.layered, m.cpu]):
            failures.append(f"{lay.name}: the fused kernel's error exceeds {fr.MARGIN} x the yardsticks: {m.line()}")
        if j >= 0 and not fr.within_margin(m.cross, [m.layered, m.cpu]):
            failures.append(f"{lay.name}: fused and layered eps differ by more than {fr.MARGIN} x the yardsticks: {m.line()}")
        if j < 0:
            # the corner pixels of eps are the corner pixels of the pooled image: the bilinear weights there are 1 and 0
            inp = cases.inputs(model, lay.name)
            for r, eps in zip(m.models, m.eps["fused"]):
                want = inp.x_rows
                for _ in range(r.pools):
                    want = F.max_pool2d(want, 2)
                want = want[:, list(r.chans)][:, :, [0, 0, -1, -1], [0, -1, 0, -1]]
                if not torch.equal(eps[:, :, [0, 0, -1, -1], [0, -1, 0, -1]], want):
                    failures.append(f"{lay.name}: route {r.pools}: a corner pixel of eps is not the pooled image's")
    assert not failures, f"{model} block {j} ({fr.BLOCKS[j] if j >= 0 else 'image'}):\n  " + "\n  ".join(failures)


# ------------------------------------------------------------------ padding
@pytest.mark.parametrize("model", ["sf0.15_19/38", "sf0.2_25/50", "sf0.15_19/38_C1"])
def test_fused_padded_and_idle_channels_never_leak(model):
    """the channel groups at the padding boundary (the last real channels of block j) and group 0: eps does not change in any
    value when the output channels of the selecting blocks that carry nothing select no input at all instead of input channel
    n % cin -- so no carrier reads a neighbour, and a padded position holds nothing"""
    sd32, lay = cases.state_dict(model), cases.LAYOUTS["one_pass_B3"]
    x = cases.inputs(model, lay.name).x.to(DEV)
    for j in cases.BLOCK_IDS:
        live, bare = list(fr.readout_models(sd32, j)), list(fr.readout_models(sd32, j, fill="none"))
        for k in sorted({0, len(live) - 1}):
            handles = [engine.UNetHandle(r.sd, DEV) for r in (live[k], bare[k])]
            eps = [fr.device_eps(h, x, lay).cpu() for h in handles]
            assert live[k].chans == bare[k].chans and torch.equal(eps[0], eps[1]), f"{model} M({j},{k}): idle channels leak into eps"
            assert eps[0].abs().max() > 0


# ------------------------------------------------------------------ rows
@pytest.mark.parametrize("j", cases.ROW_BLOCKS)
def test_fused_rows_of_readout_models(j, table):
    model = cases.ROW_MODEL
    sd32 = cases.state_dict(model)
    layouts = [cases.LAYOUTS[name] for name in cases.ROW_LAYOUTS]
    got = fr.measure_block(sd32, j, layouts, inputs_of(model, layouts), DEV)
    for lay in layouts:
        m = got[lay.name]
        table[(model, lay.name, j)] = m
        print(f"\n  {model} {lay.name} j={j}: {m.line()}")
        assert m.ok(), f"{model} block {j} {lay.name}: {m.line()}"
    # the live row of a half-empty workgroup against the same image with a live neighbour (rows 2 and 3 share a workgroup)
    half, full = cases.LAYOUTS["one_pass_B3"], fr.Layout("one_pass_B4", 4, 1, 0, 1, cases.LAYOUTS["one_pass_B3"].conds + ((23, COND_ONE),))
    x3 = cases.inputs(model, half.name).x
    x4 = torch.cat([x3, x3[1:2]]).to(DEV)
    for r in fr.readout_models(sd32, j):
        h = engine.UNetHandle(r.sd, DEV)
        a, b = fr.device_eps(h, x3.to(DEV), half), fr.device_eps(h, x4, full)
        assert torch.equal(a.view(torch.int32), b[:3].view(torch.int32)), f"{model} M({j},{r.k}): a row depends on its workgroup's other row"
        assert torch.equal(b[3].view(torch.int32), b[1].view(torch.int32))


# ------------------------------------------------------------------ loop mode
@pytest.mark.parametrize("n_pass", [1, 2])
@pytest.mark.parametrize("j", cases.LOOP_BLOCKS)
def test_fused_loop_step_equals_forward_plus_update_on_readout_models(j, n_pass):
    """one LOOP step against forward + dt_cfg_update (as test_hip_fused.py::test_fused_forward_equals_first_loop_step, whose
    update arithmetic is shared): ties the loop's image-slot indexing to the forwards checked above.  B = 5: the last workgroup
    is half empty, and with two passes a workgroup holds rows of both."""
    model = cases.LOOP_MODEL
    sd32, C = cases.state_dict(model), cases.MODELS[model].C
    B, E = 5, C * 256
    g = torch.Generator().manual_seed(80 + j)
    x_T, z = torch.randn(B, E, generator=g).to(DEV), torch.randn(B + 7, E, generator=g).to(DEV)
    coef = (1.02, 0.07, 0.05)
    for r in fr.readout_models(sd32, j):
        h = engine.UNetHandle(r.sd, DEV)
        assert h.fused_active(16, 16)
        tb = h.time_bias([30] * n_pass, [COND_NONE, COND_ONE][:n_pass])
        traj = torch.empty(2, B, E, device=DEV)
        traj[0] = x_T
        h.sample(RULE_PSAMPLE, traj, 16, 16, tb, n_pass, [coef], [True], z=z, w_scalar=2.5)
        eps = h.forward(x_T.reshape(B, C, 16, 16), tb, n_pass, B)
        eps_c = eps[B:].reshape(B, E) if n_pass == 2 else None
        want = engine.cfg_update(RULE_PSAMPLE, x_T, eps[:B].reshape(B, E), eps_c, z, coef, True, w_scalar=2.5)
        assert torch.equal(traj[1].view(torch.int32), want.view(torch.int32)), f"{model} M({j},{r.k}) n_pass {n_pass}: loop step differs from forward + update"
        assert not torch.equal(traj[1], traj[0]) and eps.abs().max() > 0


# ------------------------------------------------------------------ random models
def test_fused_blocks_of_randomised_models():
    """tools/fuzz_fused.py's block mode: three further random models (size factor, image channels, weights seed, block j and a
    one-pass batch of 1 .. 6 rows drawn at random) under the criterion above (a child process: the fuzzer is also a
    command-line tool; no cases of its tolerance-only comparison, which test_hip_fused.py runs)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_fused.py"), "0", "7", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "block draws ok 3" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
