"""Joint launch plans against float64: conv1 x conv2 pairs of the decoder blocks, the committed plan table, tuned plans.

tests/test_hip_conv_blocks.py pins one slot at a time on top of the heuristic plan; the product runs 15 pinned slots at once
(plans/gfx950.json, or dt_unet_autotune), and resolve_forward derives facts from PAIRS of slots.  The fact checked here is
concat_in_place[j]: where a decoder block's conv1 is a strip kind and its conv2 a strip kind with the 1x1 skip folded,
upcat_kernel writes the upsampled half of the concat only, and conv1 and the folded skip walk read the 16-channel chunks
>= cc_a from the encoder's output.  The helpers, references and tolerances are test_hip_conv_blocks's, unchanged.

1. test_decoder_conv_pairs_vs_float64: for dec3, dec2, dec1 (j = 5, 6, 7)
     set a  every admissible strip conv1 (kinds 3, 4, 5, every tile, every split count that survives resolution), each with
            conv2 = strip 64 x 64 +skip and, where n_p % 128 == 0, strip32 256 x 64 +skip (the pair kernel);
     set b  every admissible strip conv2 with the skip folded, each with conv1 = stripk 64 x 64 at the deepest split the layer
            admits (the K-split walk crosses the source boundary) and with conv1 = split-bf16 64 x 64 (the concat is not in
            place: the same conv2 launch reads its skip operand from the concat buffer).
   Per pair, on a default handle and on one created under DT_NO_CONCAT_IN_PLACE=1: both reports read back as pinned; the skip
   half of the concat buffer (dt_unet_debug_activation, which = 9 .. 11) is all NaN after the NaN-poisoned forward exactly when
   the rule, restated here (concat_in_place), says so, and never on the switched handle; block j's output and eps agree bit for
   bit between the handles; block j passes check_block against float64, is poison-invariant, has zero padding channels; blocks
   upstream are the heuristic run's, bit for bit; eps is finite and poison-invariant; for dec1 in set b the head-fusion rerun
   of test_hip_conv_blocks.  Every strip kind must have run as conv1 with the concat in place on every tile its channel
   count admits.

     case                       H x W    rows  pairs admitted  run  in place  refused at launch
     A_sf1.0_16px_B5           16 x 16   10        390         390     351    -
     B_sf0.3_32x48_B3          32 x 48    6        266         266     232    -
     C_sf0.5_mixed_B7_single2  16 x 16   12        303         303     269    -

   (The case's min_launches is the pairs run, rounded down to the ten.  A deliberately wrong cc_a, off by one in run_block,
   fails all three cases: 2491 / 1872 / 1899 failed checks.)

2. test_committed_plan_replayed_whole_vs_float64: every entry of plans/gfx950.json applied whole (all its slots, one
   set_precision before them) at its own H x W on a few images, read back unchanged; NaN / 1e30 poison invariance of every
   block, check_block of every block against float64 from its own upstream outputs, eps finite; head fusion on: the stored
   blocks bit-identical, eps to REL_L2 per row; the handle under DT_NO_CONCAT_IN_PLACE=1 bit-identical throughout.

3. test_tuned_plan_is_correct_and_replays: dt_unet_autotune on two small shapes; the plan it leaves is tuned on every slot,
   replays unchanged and bit-identically on a fresh handle and from DT_TUNE_CACHE, and passes the checks of part 2.

Measured on one MI355X: per-kind maxima of err / S in units of 2^-24 over part 1 (a pair counts for the kinds of both of
its convolutions): split-bf16 0.24, strip 0.20, strip32 0.24, stripk 0.20 (per-image relative L2 at most 4.7e-7, RMS of
err / S at most 0.034); over the 24 table entries the largest err / S of any block is 0.61 (the 16 / 32-channel model; 0.20
to 0.53 for the others); the tuned plans 0.20 and 0.39.  Wall time of the module 6.1 s: part 1 2.1 / 0.7 / 0.6 s per case,
a table entry 0.02 to 0.2 s, a tuned shape 0.13 / 0.34 s.
"""
from collections import defaultdict

import pytest
import torch

from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd._hip import HipLibraryError, check
from test_hip_conv_blocks import (C_TAU, POISONS, REL_L2, RMS_C, SLOT_NAMES, Case, Runner, bits, block_references, check_block,
                                  dec1_head_fuses, level, row_temb)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCH = "DT_NO_CONCAT_IN_PLACE"        # read by dt_unet_create
STRIP_KINDS = (3, 4, 5)
# the strip forms (csrc/dt_conv_forms.h: DT_CONV_FORMS_STRIP, _STRIP2, _STRIPK)
STRIP_TILES = {3: ((256, 64), (128, 128), (128, 64), (64, 128), (64, 64)),
               4: ((256, 64), (128, 128), (128, 64), (64, 128), (64, 64)),
               5: ((64, 128), (64, 64), (128, 64))}
SIZE_FACTORS = (0.05, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.75, 0.8, 0.9, 1.0)


@pytest.fixture(scope="module")
def cpu_threads():
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(old, 16)))
    yield
    torch.set_num_threads(old)


@pytest.fixture(scope="module")
def stats():
    """part 1, per launch kind: the largest err / S (2^-24), per-image relative L2 and RMS of err / S (2^-24), pairs"""
    table = defaultdict(lambda: [0.0, 0.0, 0.0, 0])
    yield table
    print("\nper-kind maxima over the decoder pairs: kind: (max err/S [2^-24], max per-image rel L2, max per-image RMS err/S "
          "[2^-24], pairs)")
    for kind in sorted(table):
        r, l2, rms, n = table[kind]
        print(f"  {_hip.KIND_NAMES.get(kind, kind)}: ({r:.3f}, {l2:.3e}, {rms:.4f}, {n})")


def state_dicts(models, sf):
    sd32 = {k: v.float() for k, v in models(sf).state_dict().items() if v.dtype.is_floating_point}
    return sd32, {k: v.double() for k, v in sd32.items()}


class PlanRunner(Runner):
    """test_hip_conv_blocks.Runner that pins several slots after ONE set_precision; in_place=False: the handle is created
    under DT_NO_CONCAT_IN_PLACE=1"""

    def __init__(self, c, sd32, monkeypatch, in_place=True):
        if not in_place:
            monkeypatch.setenv(SWITCH, "1")
        try:
            super().__init__(c, sd32)
        finally:
            monkeypatch.delenv(SWITCH, raising=False)
        self.key = (self.rows, c.H, c.W, c.B, c.single)

    def pin_plan(self, entries):
        """fresh heuristic plan + every [block, slot, bm, bn, splits, kind, fuse] of entries; raises where one is refused"""
        h, c = self.h, self.c
        h.set_precision(_hip.PREC_AUTO)
        for j, slot, bm, bn, sp, kind, fuse in entries:
            h.set_conv_choice(self.rows, c.H, c.W, j, slot, bm, bn, sp, kind, fuse, images=c.B, single=c.single)

    def pin_pair(self, j, c1, c2):
        """both 3x3 slots of block j; False where the library refuses one"""
        try:
            self.pin_plan([(j, 1) + tuple(c1), (j, 2) + tuple(c2)])
        except HipLibraryError:
            return False
        return True

    def plan(self):
        """the launches of the case's shape as plan entries, and whether every one of them is tuned"""
        ch = list(self.h._choices(self.key))
        return [list(e[:7]) for e in ch], all(e[7] for e in ch)

    def skip_half(self, j):
        """the encoder's half of the concat that decoder block j reads"""
        cat = self.h.debug_activation(self.rows, self.c.H, self.c.W, 9 + j - 5)
        up_p = -(-self.couts[j - 1] // 16) * 16         # the upsampled half: block j - 1's padded channels
        assert cat.shape[1:3] == level(self.c, j) and cat.shape[3] == up_p + -(-self.couts[8 - j] // 16) * 16, cat.shape
        return cat[..., up_p:]

    def poisoned(self, value, blocks):
        """(status, block outputs, eps) of one forward over a workspace and eps filled with value"""
        status = self.poisoned_forward(value)
        if status != 0:
            return status, None, None
        return 0, [self.act(b).clone() for b in blocks], self.eps.clone()


def concat_in_place(rep1, rep2):
    """resolve_forward: a decoder block (its skip is always a convolution: 2 c inputs, c outputs) leaves the concat's skip half
    in the encoder's output when conv1 is a strip launch and conv2 a strip launch with the skip folded"""
    return rep1[3] & 7 >= 3 and rep2[3] & 7 >= 3 and bool(rep2[3] & 8)


def rel_l2_rows(a, b):
    a, b = a.double(), b.double()
    return ((a - b).flatten(1).norm(dim=1) / b.flatten(1).norm(dim=1)).max().item()


def block_failures(where, res, differs):
    bad, ratio, rel, pad, rms = res
    out = []
    if differs:
        out.append(f"{where}: block output differs between NaN- and 1e30-poisoned workspaces")
    if bad:
        out.append(f"{where}: |err| > {C_TAU} * 2^-24 * S (max err/S = {ratio * 2 ** 24:.2f} * 2^-24)")
    if not rel <= REL_L2:
        out.append(f"{where}: per-image relative L2 error {rel:.3e} > {REL_L2:.0e}")
    if not rms * 2 ** 24 <= RMS_C:
        out.append(f"{where}: per-image RMS of err/S {rms * 2 ** 24:.3f} * 2^-24 > {RMS_C} * 2^-24")
    if pad:
        out.append(f"{where}: nonzero padding channels")
    return out


def heuristic_base(run, what):
    """the heuristic plan's block outputs and eps under both poisons, checked to be poison-invariant; the first is returned"""
    run.h.ensure_plan(*run.key, tune=False)
    run.h.set_precision(_hip.PREC_AUTO)
    base = []
    for value in POISONS:
        status, acts, eps = run.poisoned(value, range(8))
        check(status, "dt_unet_forward")
        base.append((acts, eps))
    for j in range(8):
        assert torch.equal(bits(base[0][0][j]), bits(base[1][0][j])), f"{what}: heuristic plan, {engine.BLOCK_NAMES[j]} reads unwritten memory"
    assert torch.equal(bits(base[0][1]), bits(base[1][1])) and torch.isfinite(base[0][1]).all(), f"{what}: heuristic plan, eps"
    return base[0]


def references(run, sd32, sd64, acts):
    """{j: (ref64, S)} on the device, from the device's own block outputs `acts`"""
    a64 = [a[..., :cout].permute(0, 3, 1, 2).double().cpu() for a, cout in zip(acts, run.couts)]
    temb = row_temb(sd32, run.conds, run.c.tb_div)
    return {j: (r.to(DEV), s.to(DEV)) for j, (r, s) in block_references(sd64, run.x.double()[run.imgs], a64, temb).items()}


# ------------------------------------------------------------------ 1. conv1 x conv2 pairs of the decoder blocks
#                name, sf, H, W, B, n_pass, single, tb_div, min_pairs, seed
PAIR_CASES = (
    # 8 / 16 chunks, cc_a even, N pairs; dec3 40 rows (one ragged tile), dec2 160, dec1 640: a pass boundary inside a 256-row tile
    Case("A_sf1.0_16px_B5", 1.0, 16, 16, 5, 2, 0, 5, 390, 41),
    # 76 -> 80 channels: cc_a = 5 is odd, the source boundary falls inside a K = 32 step and inside stripk's chunk groups;
    # pictures of 16 x 24, 8 x 12 and 4 x 6: every tile takes the halo W + 1
    Case("B_sf0.3_32x48_B3", 0.3, 32, 48, 3, 2, 0, 1, 260, 42),
    Case("C_sf0.5_mixed_B7_single2", 0.5, 16, 16, 7, 2, 2, 1, 300, 43),
)
#                (bm, bn, splits, kind + 8 fuse) as dt_unet_conv_choice reports them
CONV2_64 = (64, 64, 1, 3 + 8)        # set a's companions: strip 64 x 64 +skip, and the pair kernel's launch
CONV2_PAIR = (256, 64, 1, 4 + 8)
CONV1_GEMM = (64, 64, 1, 1)          # set b's companion that keeps the concat out of place


def decoder_pairs(run, j, found):
    """[(set, conv1 key, conv2 key)] of block j; a key is Runner.admissible's: (j, slot, bm, bn, splits, kind + 8 fuse)"""
    conv1 = sorted(k for k in found if k[:2] == (j, 1))
    conv2 = sorted(k for k in found if k[:2] == (j, 2))
    strip1 = [k for k in conv1 if k[5] >= 3]
    fused2 = [k for k in conv2 if k[5] & 8 and k[5] & 7 >= 3]
    n_p = -(-run.couts[j] // 64) * 64
    comp2 = [(j, 2) + CONV2_64] + ([(j, 2) + CONV2_PAIR] if n_p % 128 == 0 else [])
    deepest = max(k[4] for k in strip1 if k[2:4] == (64, 64) and k[5] == 5)
    comp1 = [(j, 1, 64, 64, deepest, 5), (j, 1) + CONV1_GEMM]
    for k in comp1 + comp2:
        assert k in found, f"{engine.BLOCK_NAMES[j]}: companion {k} is not admissible"
    return [("a", k1, k2) for k1 in strip1 for k2 in comp2] + [("b", k1, k2) for k2 in fused2 for k1 in comp1]


def describe(key):
    return f"{_hip.KIND_NAMES[key[5] & 7]} {key[2]}x{key[3]} s{key[4]}{' +skip' if key[5] & 8 else ''}"


@pytest.mark.parametrize("case", PAIR_CASES, ids=[c.name for c in PAIR_CASES])
def test_decoder_conv_pairs_vs_float64(case, models, monkeypatch, cpu_threads, stats):
    c = case
    sd32, sd64 = state_dicts(models, c.sf)
    run = PlanRunner(c, sd32, monkeypatch)
    off = PlanRunner(c, sd32, monkeypatch, in_place=False)
    base_acts, _ = heuristic_base(run, c.name)
    refs = references(run, sd32, sd64, base_acts)
    off.h.ensure_plan(*off.key, tune=False)

    found = run.admissible(range(5, 8), [1, 2])
    pairs = [p for j in range(5, 8) for p in decoder_pairs(run, j, found)]
    failures, ran, refused = [], 0, []
    in_place_ran = defaultdict(set)        # block -> {(kind, bm, bn)} of conv1 launches that ran with the concat in place
    n_in_place, head_runs = 0, [0, 0]
    for which, k1, k2 in pairs:
        j = k1[0]
        what = f"{engine.BLOCK_NAMES[j]} [{which}] conv1 {describe(k1)} (request {found[k1]}) + conv2 {describe(k2)} (request {found[k2]})"
        expect = concat_in_place(k1[2:], k2[2:])
        outs, nan_half, flags, status = [], None, [], 0
        assert run.pin_pair(j, found[k1], found[k2]) and off.pin_pair(j, found[k1], found[k2]), what
        for r in (run, off):
            reps = r.report(j, 1), r.report(j, 2)
            assert (reps[0][:4], reps[1][:4]) == (k1[2:], k2[2:]) and reps[0][4] == reps[1][4] == 1, f"{what}: reports {reps}"
        for value in POISONS:
            status, acts, eps = run.poisoned(value, [j])
            if status < 0:
                break
            check(status, f"dt_unet_forward ({what})")
            outs.append((acts[0], eps))
            if nan_half is None:           # (the first poison is NaN)
                nan_half = torch.isnan(run.skip_half(j)).all().item()
            flags += [(bits(run.act(u)) != bits(base_acts[u])).any() for u in range(j)]
        if status < 0:
            refused.append((k1, k2))       # the launcher refuses a choice the rules resolve to
            continue
        ran += 1
        # the handle without the in-place concat: the same launches, the skip half read from the concat buffer
        status, acts_off, eps_off = off.poisoned(POISONS[0], [j])
        check(status, f"dt_unet_forward ({what}, {SWITCH}=1)")
        if torch.isnan(off.skip_half(j)).all().item():
            failures.append(f"{what}: {SWITCH}=1, the concat's skip half is unwritten")
        if nan_half != expect:
            failures.append(f"{what}: the concat's skip half is {'un' if nan_half else ''}written, the rule says in place = {expect}")
        if not torch.equal(bits(outs[0][0]), bits(acts_off[0])):
            diff = (outs[0][0].double() - acts_off[0].double()).abs().max().item()
            failures.append(f"{what}: block output differs from the {SWITCH}=1 handle's (max {diff:.3e})")
        if not torch.equal(bits(outs[0][1]), bits(eps_off)):
            failures.append(f"{what}: eps differs from the {SWITCH}=1 handle's")
        for r, tag in ((run, "default"), (off, SWITCH)):
            reps = r.report(j, 1), r.report(j, 2)
            if (reps[0][:4], reps[1][:4]) != (k1[2:], k2[2:]) or reps[0][4] != 1 or reps[1][4] != 1:
                failures.append(f"{what}: [{tag}] the reports after the forward show {reps}, not the pins")
        ref, S = refs[j]
        res = check_block(outs[0][0], ref, S, run.couts[j]).tolist()
        failures += block_failures(what, res, (bits(outs[0][0]) != bits(outs[1][0])).any().item())
        if not torch.equal(bits(outs[0][1]), bits(outs[1][1])) or not torch.isfinite(outs[0][1]).all():
            failures.append(f"{what}: eps differs between poisons or is not finite")
        if flags and torch.stack(flags).any().item():
            failures.append(f"{what}: a block upstream of the pinned one changed")
        for kind in {k1[5] & 7, k2[5] & 7}:
            st = stats[kind]
            st[0], st[1], st[2], st[3] = max(st[0], res[1] * 2 ** 24), max(st[1], res[2]), max(st[2], res[4] * 2 ** 24), st[3] + 1
        if nan_half and expect:
            n_in_place += 1
            in_place_ran[j].add((k1[5], k1[2], k1[3]))
        if j == 7 and which == "b":
            # head fusion on (the product's setting): dec1.conv2's epilogue evaluates the head where the rule says so
            run.h.set_head_fusion(True)
            on = []
            for value in POISONS:
                check(run.poisoned_forward(value), f"dt_unet_forward ({what}, head fusion on)")
                on.append((run.eps.clone(), torch.isnan(run.act(7)).all().item()))
            run.h.set_head_fusion(False)
            if not torch.equal(bits(on[0][0]), bits(on[1][0])) or not torch.isfinite(on[0][0]).all():
                failures.append(f"{what}: head fusion on, eps differs between poisons or is not finite")
            unstored = dec1_head_fuses(run, k2[2:])
            if on[0][1] != unstored:
                failures.append(f"{what}: head fusion on, dec1's output is {'not ' if on[0][1] else ''}stored")
            rel_eps = rel_l2_rows(on[0][0], outs[0][1])
            if not rel_eps <= REL_L2:
                failures.append(f"{what}: eps with head fusion on differs by {rel_eps:.3e} (relative L2, worst row)")
            head_runs[0] += 1
            head_runs[1] += unstored

    print(f"\n{c.name}: {len(pairs)} pairs admitted, {ran} run ({n_in_place} with the concat in place), refused at launch: "
          f"{refused}; dec1 reruns with head fusion on: {head_runs[0]} ({head_runs[1]} with the head in the epilogue)")
    print("  conv1 strip tiles run with the concat in place: " + "; ".join(
        f"{engine.BLOCK_NAMES[j]} " + ", ".join(f"{_hip.KIND_NAMES[k]} " + " ".join(f"{bm}x{bn}" for kk, bm, bn in sorted(t) if kk == k)
                                                for k in STRIP_KINDS) for j, t in sorted(in_place_ran.items())))
    assert not failures, f"{c.name}: {len(failures)} failures:\n  " + "\n  ".join(failures[:40])
    # the one choice the rules admit and the launcher refuses: stripk's 64 x 64 tile on picture rows of more than 31 pixels
    for k1, k2 in refused:
        assert level(c, k1[0])[1] > 31 and any((k[5] & 7, k[2], k[3]) == (5, 64, 64) for k in (k1, k2)), f"{c.name}: pair {(k1, k2)} refused"
    for j in range(5, 8):
        n_p, w = -(-run.couts[j] // 64) * 64, level(c, j)[1]
        want = {(k, bm, bn) for k in STRIP_KINDS for bm, bn in STRIP_TILES[k] if n_p % bn == 0 and not ((k, bm, bn) == (5, 64, 64) and w > 31)}
        assert in_place_ran[j] == want, f"{c.name}: {engine.BLOCK_NAMES[j]} ran in place {sorted(in_place_ran[j])}, its channels admit {sorted(want)}"
    assert ran >= c.min_launches, f"{c.name}: only {ran} pairs ran"


# ------------------------------------------------------------------ whole plans: the checks parts 2 and 3 share
def check_whole_plan(run, off, entries, sd32, sd64, what):
    """The pinned plan `entries` on run's handle (and on off's, created without the in-place concat) against float64, every
    block from its own upstream outputs.  Returns (failures, largest err / S over the blocks in units of 2^-24, head-off block
    outputs, head-on eps, the decoder blocks whose concat was in place)."""
    failures = []
    run.h.set_head_fusion(False)
    outs, in_place = [], None
    for value in POISONS:
        status, acts, eps = run.poisoned(value, range(8))
        check(status, f"dt_unet_forward ({what})")
        outs.append((acts, eps))
        if in_place is None:               # (the first poison is NaN) the state resolve_forward derives from the pairs of slots
            in_place = [j for j in range(5, 8) if torch.isnan(run.skip_half(j)).all().item()]
    kinds = {(e[0], e[1]): (e[2], e[3], e[4], e[5] + 8 * e[6]) for e in entries}
    rule = [j for j in range(5, 8) if concat_in_place(kinds[(j, 1)], kinds[(j, 2)])]
    if in_place != rule:
        failures.append(f"{what}: the concat's skip half is unwritten for blocks {in_place}, the rule says {rule}")
    if not torch.equal(bits(outs[0][1]), bits(outs[1][1])) or not torch.isfinite(outs[0][1]).all():
        failures.append(f"{what}: eps differs between poisons or is not finite")
    refs = references(run, sd32, sd64, outs[0][0])
    worst = 0.0
    for j in range(8):
        ref, S = refs[j]
        res = check_block(outs[0][0][j], ref, S, run.couts[j]).tolist()
        worst = max(worst, res[1] * 2 ** 24)
        failures += block_failures(f"{what}, {engine.BLOCK_NAMES[j]}", res, (bits(outs[0][0][j]) != bits(outs[1][0][j])).any().item())
    # head fusion on, the product's setting
    run.h.set_head_fusion(True)
    on = []
    for value in POISONS:
        status, acts, eps = run.poisoned(value, range(8))
        check(status, f"dt_unet_forward ({what}, head fusion on)")
        on.append((acts, eps))
    run.h.set_head_fusion(False)
    if not torch.equal(bits(on[0][1]), bits(on[1][1])) or not torch.isfinite(on[0][1]).all():
        failures.append(f"{what}: head fusion on, eps differs between poisons or is not finite")
    for j in range(8):
        a = on[0][0][j]
        if j in (0, 7) and torch.isnan(a).all():
            continue                           # not stored with head fusion on: enc1 under skip_out, dec1 under the fused head
        if not torch.equal(bits(a), bits(outs[0][0][j])):
            failures.append(f"{what}: head fusion on changes {engine.BLOCK_NAMES[j]}")
    rel_eps = rel_l2_rows(on[0][1], outs[0][1])
    if not rel_eps <= REL_L2:
        failures.append(f"{what}: eps with head fusion on differs by {rel_eps:.3e} (relative L2, worst row)")
    # the handle without the in-place concat
    off.pin_plan(entries)
    got, tuned = off.plan()
    if got != [list(e) for e in entries] or not tuned:
        failures.append(f"{what}: the {SWITCH}=1 handle reads the plan back as {got}")
    status, acts, eps = off.poisoned(POISONS[0], range(8))
    check(status, f"dt_unet_forward ({what}, {SWITCH}=1)")
    for j in range(8):
        if not torch.equal(bits(acts[j]), bits(outs[0][0][j])):
            failures.append(f"{what}: {engine.BLOCK_NAMES[j]} differs from the {SWITCH}=1 handle's")
    if not torch.equal(bits(eps), bits(outs[0][1])):
        failures.append(f"{what}: eps differs from the {SWITCH}=1 handle's")
    return failures, worst, outs[0][0], on[0][1], in_place


# ------------------------------------------------------------------ 2. every entry of the committed plan table
TABLE_KEYS = sorted(engine._Plans.table())


def table_shape(key):
    """the small batch an entry is replayed on: (H, W, images, passes, single-pass images) from `...|rows x H x W|images/single`"""
    shape, split = key.split("|")[-2:]
    H, W = (int(v) for v in shape.split("x")[1:])
    if split == "256/64":
        return H, W, 7, 2, 1
    if split == "512/64":
        return H, W, 9, 2, 3
    if split == "256/0":
        return H, W, 5, 2, 0
    assert (shape, split) == ("256x32x32", "128/0"), key
    return H, W, 3, 2, 0


@pytest.fixture(scope="module")
def model_of_key(models):
    """{the model part of a plan key: size factor}, from a handle of every size factor (the key is the handle's own)"""
    out = {}
    for sf in SIZE_FACTORS:
        h = engine.UNetHandle(state_dicts(models, sf)[0], DEV)
        out.setdefault(h.plan_key(0, 0, 0, 0, 0).rsplit("|", 2)[0], sf)
    return out


def test_plan_table_has_entries():
    assert TABLE_KEYS, f"{engine.PLAN_TABLE} holds no plan"


@pytest.mark.parametrize("key", TABLE_KEYS, ids=[k.split("|", 4)[-1] for k in TABLE_KEYS])
def test_committed_plan_replayed_whole_vs_float64(key, models, model_of_key, monkeypatch, cpu_threads):
    entries = engine._Plans.table()[key]
    model = key.rsplit("|", 2)[0]
    assert model in model_of_key, f"no size factor of {SIZE_FACTORS} has the model of {key}"
    sf = model_of_key[model]
    H, W, B, n_pass, single = table_shape(key)
    c = Case(f"table_sf{sf}", sf, H, W, B, n_pass, single, 1, 0, 50 + TABLE_KEYS.index(key))
    sd32, sd64 = state_dicts(models, sf)
    run = PlanRunner(c, sd32, monkeypatch)
    off = PlanRunner(c, sd32, monkeypatch, in_place=False)
    assert run.h.plan_key(*run.key).rsplit("|", 2)[0] == model
    run.pin_plan(entries)                  # (a refused entry raises)
    got, tuned = run.plan()
    assert got == [list(e) for e in entries] and tuned, f"{key}: applied {entries}, read back {got} (tuned {tuned})"
    failures, worst, _, _, in_place = check_whole_plan(run, off, entries, sd32, sd64, f"sf {sf} {run.rows}x{H}x{W} {B}/{single}")
    print(f"\n{key}: sf {sf}, {run.rows} rows ({B} images, {single} single-pass), max err/S over the blocks {worst:.3f} * 2^-24, "
          f"concat in place: {[engine.BLOCK_NAMES[j] for j in in_place]}")
    assert not failures, f"{key}: {len(failures)} failures:\n  " + "\n  ".join(failures[:40])


# ------------------------------------------------------------------ 3. what the tuner leaves behind
TUNE_CASES = (
    Case("T_sf0.5_16px_B5", 0.5, 16, 16, 5, 2, 0, 1, 0, 81),
    Case("T_sf1.0_32px_B3", 1.0, 32, 32, 3, 2, 0, 1, 0, 82),
)


@pytest.mark.parametrize("case", TUNE_CASES, ids=[c.name for c in TUNE_CASES])
def test_tuned_plan_is_correct_and_replays(case, models, monkeypatch, tmp_path, cpu_threads):
    c = case
    sd32, sd64 = state_dicts(models, c.sf)
    monkeypatch.setenv("DT_TUNE_CACHE", str(tmp_path / "tune_cache.json"))
    run = PlanRunner(c, sd32, monkeypatch)
    h = run.h
    h.set_head_fusion(True)                # tuned as the product runs: dec1.conv2's candidates are those that carry the head
    plan_id = h.ensure_plan(*run.key, tune=True, warm=lambda: check(run.forward(), "dt_unet_forward"))
    assert plan_id.startswith("tuned:"), plan_id
    plan, tuned = run.plan()
    print(f"\n{c.name}: {plan_id}: " + " ".join(f"{engine.BLOCK_NAMES[e[0]]}.{SLOT_NAMES[e[1]]}={e[2]}x{e[3]}s{e[4]}k{e[5]}{'+skip' if e[6] else ''}"
                                                for e in plan))
    assert tuned and plan == h._read_plan(*run.key[:3]), f"{c.name}: not every launched slot is tuned: {list(h._choices(run.key))}"

    # the plan applied to a fresh handle is accepted, read back unchanged, and computes the same bits
    fresh = PlanRunner(c, sd32, monkeypatch)
    assert fresh.h._apply_plan(fresh.key, plan), f"{c.name}: a fresh handle refuses part of {plan}"
    assert fresh.plan() == (plan, True), f"{c.name}: a fresh handle reads {fresh.plan()} back"
    off = PlanRunner(c, sd32, monkeypatch, in_place=False)
    failures, worst, acts, eps_on, in_place = check_whole_plan(run, off, plan, sd32, sd64, c.name)
    print(f"{c.name}: max err/S over the blocks {worst:.3f} * 2^-24, concat in place: {[engine.BLOCK_NAMES[j] for j in in_place]}")
    assert not failures, f"{c.name}: {len(failures)} failures:\n  " + "\n  ".join(failures[:40])
    assert run.plan() == (plan, True), f"{c.name}: the tuned plan moved: {run.plan()}"
    status, f_acts, _ = fresh.poisoned(POISONS[0], range(8))          # (a Runner starts with head fusion off)
    check(status, "dt_unet_forward (replayed plan)")
    for j in range(8):
        assert torch.equal(bits(f_acts[j]), bits(acts[j])), f"{c.name}: {engine.BLOCK_NAMES[j]} of the replayed plan differs from the tuned handle's"
    fresh.h.set_head_fusion(True)
    check(fresh.poisoned_forward(POISONS[0]), "dt_unet_forward (replayed plan, head fusion on)")
    assert torch.equal(bits(fresh.eps), bits(eps_on)), f"{c.name}: eps of the replayed plan differs from the tuned handle's"

    # a third handle finds the plan in the cache the tuning run wrote
    third = PlanRunner(c, sd32, monkeypatch)
    cache_id = third.h.ensure_plan(*third.key)
    assert cache_id == "cache:" + plan_id.split(":")[1], (cache_id, plan_id)
    assert third.plan() == (plan, True), f"{c.name}: the cached plan reads back as {third.plan()}"
