"""The readout surgery of tests/fused_readout.py, without a GPU: that it is exact, that it reads every channel, that the
inputs of tests/fused_readout_cases.py are not degenerate, and that the criterion of tests/test_hip_fused_blocks.py is sharp.

Sharpness: the fp32 CPU oracle is evaluated with one deliberate fault in one block -- the faults a kernel that overlays LDS
buffers, splits taps over waves, pools by lane shuffles and masks out-of-picture taps could have -- and the criterion
(error against float64 greater than MARGIN x the unbroken fp32 oracle's error) must reject each at its own block.  The
same faults end to end, under the rtol 1e-4 + atol 2e-5 of tests/test_hip_fused.py, are printed (pytest -s), not asserted:

  fault (sf 0.2, 25 / 50 channels, one pass, B = 3)          faulty / unbroken rel L2    end to end: max err, 1e-4 bound
  (a)  tap dropped on a border row, 2x2 level (enc4.conv2)   1.9e-02 / 1.1e-07  enc4      4.3e-03   fails
  (a4) the same for one quad of input channels               3.4e-03 / 1.1e-07  enc4      5.2e-04   fails
  (b)  two channels of dec2's skip source swapped            6.0e-02 / 1.7e-07  dec2      6.4e-03   fails
  (c)  a pool window's max over three of four elements       9.4e-04 / 1.0e-07  enc3      4.1e-04   fails
  (d)  time-bias row r used for row r + 1 (dec3)             5.9e-02 / 2.1e-07  dec3      1.4e-02   fails
  (e)  one (tap, 16-channel chunk) product twice, 1x1 level  7.7e-03 / 1.3e-07  bottlen.  1.1e-03   fails
  (f)  one 16-channel chunk of enc4.conv2 read as bf16       1.0e-04 / 1.1e-07  enc4      1.6e-05   PASSES
  (g)  fault (c) with the second largest element dropped     no value changes: the control, accepted

On these seeded random models the five structural faults, in the forms above, are large enough to miss the end-to-end bound as
well (by factors of 4 to 140; sf 0.1, 0.15 and 0.25 give the same picture) -- what the block criterion adds for them is the
distance, four to five orders of magnitude instead of one, and the name of the block.  A loss of precision in one K chunk,
(f), passes the end-to-end bound on three of the four models and misses the block criterion by a factor of 200.
"""
import pytest
import torch
import torch.nn.functional as F

import fused_readout as fr
import fused_readout_cases as cases
from oracle import unet_ref

BLOCKS = fr.BLOCKS
MIN_NORM = 1e-2          # a row's readouts, concatenated: "bounded away from 0" (they are O(1) numbers; measured minimum below)
MIN_LIVE = 0.75          # share of block j's real channels that are not identically zero (tests/test_hip_inception.py's share)


@pytest.fixture(scope="module", autouse=True)
def cpu_threads():
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(old, 16)))
    yield
    torch.set_num_threads(old)


def same64(a, b):
    """equal up to the float64 rounding of the bilinear upsamples: ATen's CPU kernel contracts its blend differently from one
    chunk of its parallel loop to the next, so the same plane upsampled inside tensors of different channel counts differs in
    the last bit (measured: at most 1.6 * 2^-52 of the largest magnitude after four upsamples; pools, selections, concats and
    transparent blocks are exact).  Nine orders of magnitude below the fp32 errors the device test measures."""
    return a.shape == b.shape and float((a - b).abs().max()) <= 2.0 ** -49 * float(b.abs().max())


def source(inp, j, wide=True):
    """what M(j, k) reads: block j's output, the image for j = -1"""
    if j < 0:
        return inp.x_rows.double() if wide else inp.x_rows
    return (inp.acts64 if wide else inp.acts32)[j]


# ------------------------------------------------------------------ exactness and coverage
@pytest.mark.parametrize("model", list(cases.MODELS))
def test_surgery_is_exact_in_float64_and_reads_every_channel(model):
    """forward64 of M(j, k), evaluated from the image with no shortcut, IS the readout (select, pool, bilinear upsamples) of
    forward64's own block-j output of the unchanged model; so is the shortcut the device test takes
    (blocks 0 .. j from the unchanged model's outputs); and what the non-carrier channels select changes nothing.  "Number
    for number" up to the last bits of the float64 upsamples: see same64."""
    sd32, m = cases.state_dict(model), cases.MODELS[model]
    inp = cases.inputs(model, "one_pass_B3")
    x64, t64 = inp.x_rows.double(), inp.temb.double()
    n_models = 0
    for j in cases.BLOCK_IDS:
        read = set()
        width = fr.block_width(sd32, j)
        for r, bare in zip(fr.readout_models(sd32, j), fr.readout_models(sd32, j, fill="none")):
            assert len(r.chans) == m.C and r.chans == bare.chans and all(0 <= c < width for c in r.chans)
            want = fr.readout(source(inp, j), r)
            full, acts = fr.forward64(fr.widen(r.sd), x64, t64)
            assert same64(full, want), f"{model} M({j},{r.k}): forward64 is not the readout of block {j}"
            for b in range(max(j + 1, 0)):
                assert torch.equal(acts[b], inp.acts64[b]), f"{model} M({j},{r.k}): block {b} upstream changed"
            assert same64(cases.references(model, "one_pass_B3", r)[0], want)
            assert same64(fr.forward64(fr.widen(bare.sd), x64, t64)[0], want), f"{model} M({j},{r.k}): fill changes eps"
            # the selections carry no weight but 0 and 1, no bias, and `final` exactly C ones
            fw = r.sd["final.weight"]
            assert fw.sum() == m.C and set(fw.unique().tolist()) <= {0.0, 1.0} and not r.sd["final.bias"].any()
            read.update(r.chans)
            n_models += 1
        assert read == set(range(width)), f"{model} block {j}: channels {sorted(set(range(width)) - read)} are never read"
    print(f"\n{model}: {n_models} readout models, every one exact in float64")


def test_block_chain_is_the_oracle_bit_for_bit():
    """forward_blocks on fp32 weights (the CPU yardstick of the device test) gives unet_ref.unet_forward's bits, on the
    unchanged model and on readout models"""
    model, lay = "sf0.15_19/38", cases.LAYOUTS["cfg_B4"]
    sd32, inp = cases.state_dict(model), cases.inputs(model, "cfg_B4")
    sds = [sd32] + [next(iter(fr.readout_models(sd32, j))).sd for j in (-1, 2, 6)]
    for sd in sds:
        with torch.no_grad():
            got = fr.forward_blocks(sd, inp.x_rows, inp.temb)[0]
            t = torch.full((lay.B,), lay.conds[0][0])
            want = torch.cat([unet_ref.unet_forward(sd, inp.x, t, None), unet_ref.unet_forward(sd, inp.x, t, torch.ones(lay.B, 1))])
        assert torch.equal(got, want)


# ------------------------------------------------------------------ the inputs are not degenerate
@pytest.mark.parametrize("model", list(cases.MODELS))
def test_reference_is_not_degenerate(model):
    """every (model, layout, j, row): the row's readouts have a norm away from 0 and at least 75 % of block j's real channels
    are not identically zero in them -- of the float64 reference alone, on the inputs the device test runs"""
    sd32 = cases.state_dict(model)
    layouts = cases.SWEEP_LAYOUTS + (cases.ROW_LAYOUTS if model == cases.ROW_MODEL else ())
    low_norm, low_live = float("inf"), 1.0
    for layout in layouts:
        inp = cases.inputs(model, layout)
        for j in cases.BLOCK_IDS:
            width, live, norm2 = fr.block_width(sd32, j), {}, 0.0
            for r in fr.readout_models(sd32, j):
                ref = fr.readout(source(inp, j), r)                    # (= forward64 of M(j, k): the test above)
                norm2 = norm2 + ref.flatten(1).square().sum(dim=1)
                for i, c in enumerate(r.chans):
                    live[c] = live.get(c, False) | (ref[:, i].flatten(1) != 0).any(dim=1)
            norms = norm2.sqrt()
            share = torch.stack([live[c] for c in range(width)]).double().mean(dim=0)     # per row
            low_norm, low_live = min(low_norm, float(norms.min())), min(low_live, float(share.min()))
            assert (norms >= MIN_NORM).all(), f"{model} {layout} block {j}: row norms {norms.tolist()}"
            assert (share >= MIN_LIVE).all(), f"{model} {layout} block {j}: live channel share per row {share.tolist()}"
    print(f"\n{model}: smallest row norm {low_norm:.3g}, smallest share of live channels in a row {low_live:.2f}")


# ------------------------------------------------------------------ deliberately broken fp32 evaluations
def _block(sd, name, x, temb, hook1=None, hook2=None):
    """unet_ref.block_forward with a hook on either convolution's output: hook(input, weight, output) -> output"""
    rkey = name + ".residual_conv.weight"
    res = F.conv2d(x, sd[rkey], sd[name + ".residual_conv.bias"]) if rkey in sd else x
    c1 = F.conv2d(x, sd[name + ".conv1.weight"], sd[name + ".conv1.bias"], padding=1)
    c1 = hook1(x, sd[name + ".conv1.weight"], c1) if hook1 else c1
    h = F.relu(unet_ref._bn(sd, name + ".norm1", c1))
    tb = F.relu(F.linear(temb, sd[name + ".time_mlp.weight"], sd[name + ".time_mlp.bias"]))
    h = h + tb[:, :, None, None].expand(-1, -1, h.size(2), h.size(3))
    c2 = F.conv2d(h, sd[name + ".conv2.weight"], sd[name + ".conv2.bias"], padding=1)
    c2 = hook2(h, sd[name + ".conv2.weight"], c2) if hook2 else c2
    return F.relu(unet_ref._bn(sd, name + ".norm2", c2)) + res


def _drop_tap(x, w, out):                # 2 x 2 pictures: tap (ky, kx) = (1, 0), the left neighbour, for the pixels of row 0
    wt = torch.zeros_like(w)
    wt[:, :, 1, 0] = w[:, :, 1, 0]
    out = out.clone()
    out[:, :, 0, :] -= F.conv2d(x, wt, padding=1)[:, :, 0, :]
    return out


def _drop_tap_quad(x, w, out):           # the same tap, for input channels 8 .. 11 alone
    wt = torch.zeros_like(w)
    wt[:, 8:12, 1, 0] = w[:, 8:12, 1, 0]
    out = out.clone()
    out[:, :, 0, :] -= F.conv2d(x, wt, padding=1)[:, :, 0, :]
    return out


def _chunk_twice(x, w, out):             # 1 x 1 pictures: the centre tap's product over input channels 16 .. 31, once more
    return out + F.conv2d(x[:, 16:32], w[:, 16:32, 1:2, 1:2])


def _chunk_bf16(x, w, out):              # input channels 16 .. 31 rounded to bf16 in front of every tap's product
    d = x[:, 16:32].bfloat16().float() - x[:, 16:32]
    return out + F.conv2d(d, w[:, 16:32], padding=1)


def _pool_three(rank):
    def pool(src, pooled):               # one window of row 1, channel 7: the max over the elements but the rank-th largest
        win = src[1, 7, 2:4, 4:6].flatten().sort(descending=True).values
        pooled = pooled.clone()
        pooled[1, 7, 1, 2] = torch.cat([win[:rank], win[rank + 1:]]).max()
        return pooled
    return pool


def _swap(skip):
    skip = skip.clone()
    skip[:, [5, 6]] = skip[:, [6, 5]]
    return skip


def _shift_row(temb):
    temb = temb.clone()
    temb[1] = temb[0]
    return temb


# name -> (block at fault, what is replaced there, whether any value can change at all)
FAULTS = {
    "(a) tap dropped on a border row, 2x2 level": (3, dict(hook2=_drop_tap), True),
    "(a4) the same, one quad of input channels": (3, dict(hook2=_drop_tap_quad), True),
    "(b) two channels of dec2's skip source swapped": (6, dict(skip=_swap), True),
    "(c) a pool window's max over three of four": (2, dict(pool=_pool_three(0)), True),
    "(d) time-bias row r used for row r + 1": (5, dict(temb=_shift_row), True),
    "(e) one (tap, chunk) product twice, 1x1 level": (4, dict(hook1=_chunk_twice), True),
    "(f) one chunk of enc4.conv2 read as bf16": (3, dict(hook2=_chunk_bf16), True),
    "(g) fault (c), second largest dropped": (2, dict(pool=_pool_three(1)), False),
}


def faulty_forward(sd, x, temb, at, fault):
    """forward_blocks with block ``at`` evaluated under the fault"""
    a = []
    for j in range(8):
        here = fault if j == at else {}
        if j == 0:
            xin = x
        elif j <= 4:
            xin = F.max_pool2d(a[j - 1], 2)
            xin = here["pool"](a[j - 1], xin) if "pool" in here else xin
        else:
            skip = here["skip"](a[8 - j]) if "skip" in here else a[8 - j]
            xin = torch.cat([fr._up(a[j - 1]), skip], dim=1)
        tj = here["temb"](temb) if "temb" in here else temb
        a.append(_block(sd, BLOCKS[j], xin, tj, here.get("hook1"), here.get("hook2")))
    return F.conv2d(fr._up(a[7]), sd["final.weight"], sd["final.bias"])


@pytest.mark.parametrize("model", [m for m in cases.MODELS if cases.MODELS[m].C == 3])
def test_criterion_rejects_every_deliberate_fault_at_its_block(model):
    layout = "one_pass_B3"
    sd32, inp = cases.state_dict(model), cases.inputs(model, layout)
    with torch.no_grad():
        assert torch.equal(faulty_forward(sd32, inp.x_rows, inp.temb, 0, {}), fr.forward_blocks(sd32, inp.x_rows, inp.temb)[0])
        e2e_want = fr.forward_blocks(sd32, inp.x_rows, inp.temb)[0].double()
    print(f"\n{model}, {layout}: fault: block criterion [rel L2, max-abs: faulty / unbroken fp32 oracle]; end to end under 1e-4")
    for name, (at, fault, real) in FAULTS.items():
        refs, good, bad = [], [], []
        for r in fr.readout_models(sd32, at):
            ref64, cpu32 = cases.references(model, layout, r)
            with torch.no_grad():
                broken = faulty_forward(r.sd, inp.x_rows, inp.temb, at, fault)
            refs.append(ref64), good.append(cpu32), bad.append(broken)
        ref = torch.stack(refs)
        e_good, e_bad = fr.row_errors(torch.stack(good), ref), fr.row_errors(torch.stack(bad), ref)
        rejected = not fr.within_margin(e_bad, [e_good])
        with torch.no_grad():
            e2e = (faulty_forward(sd32, inp.x_rows, inp.temb, at, fault).double() - e2e_want).abs()
        passes = bool((e2e <= 2e-5 + 1e-4 * e2e_want.abs()).all())
        print(f"  {name:46s} at {BLOCKS[at]:10s}: [{e_bad[0]:.2e}, {e_bad[1]:.2e}] / [{e_good[0]:.2e}, {e_good[1]:.2e}] "
              f"{'rejected' if rejected else 'accepted'}; end to end max err {e2e.max():.1e}: "
              f"{'PASSES' if passes else 'fails'} today's bound")
        if real:
            assert rejected, f"{model}: the criterion accepts {name} at {BLOCKS[at]}: {e_bad} against {e_good}"
        else:
            assert e_bad == e_good, f"{model}: {name} changes a value"
        # blocks upstream of the fault see nothing of it
        if at > 0 and real:
            r = next(iter(fr.readout_models(sd32, at - 1)))
            with torch.no_grad():
                assert torch.equal(faulty_forward(r.sd, inp.x_rows, inp.temb, at, fault), cases.references(model, layout, r)[1])
