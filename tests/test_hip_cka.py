"""GPU: layer-wise CKA (include/dt_hip_cka.h, engine.device_cka, UNetHandle.block_features,
analysis/metrics/representation.py) against the extended-precision yardstick tests/cka_ref64.py within tolerances derived
there, and the header's bit contracts.  Observed error over bound on an MI355X: DESIGN §9ae."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import cka_cases
import cka_ref64 as ref
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd._hip import COND_ONE
from distillation_trajectories_amd.analysis.metrics import representation
from distillation_trajectories_amd.synthetic import seeded_noise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLAB = engine.CKA_SLAB
WIDTHS = (1, 3, 17, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 5)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def features(seed, n, p, offset=1.0):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((n, p)) + offset * rs.uniform(-1, 1, size=p)).astype(np.float32)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64).numpy()


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ Gram cells
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 130])
def test_gram_cells_against_the_yardstick(n):
    """every width around the slab length in one call; 130 rows are 3 x 3 tiles with mirrored off-diagonal ones"""
    layers = [features(1000 + n + p, n, p) for p in WIDTHS]
    g = engine.device_cka_gram([dev(X) for X in layers])
    assert g.status.tolist() == [0] * len(layers)
    got = g.gram.cpu().numpy()
    worst = 0.0
    for X, K in zip(layers, got):
        assert np.array_equal(K, K.T), f"p={X.shape[1]}: the Gram is not symmetric bit for bit"
        err = np.abs((K.astype(np.longdouble) - ref.centred_gram(X)).astype(np.float64))
        bound = ref.cell_bound(X)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"n={n} p={X.shape[1]}: worst cell error / bound {float((err / bound).max()):.3g}"
        err = np.abs((K.astype(np.longdouble) - ref.exact_centred_gram(X)).astype(np.float64))     # exact means: fully independent
        assert (err <= ref.exact_mean_cell_bound(X)).all(), f"n={n} p={X.shape[1]} against the exact-mean Gram"
    print(f"gram cells n={n}: worst error / bound {worst:.3g}")


def test_layer_sums_are_what_the_header_says():
    X = features(7, 21, 300)
    g = engine.device_cka_gram([dev(X)])
    K = g.gram[0].cpu().numpy().astype(np.longdouble)
    S = g.sums[0].cpu().numpy()
    Kt = ref.off_diagonal(K)
    n, rows = 21, Kt.sum(axis=1)
    want = [ref.inner(K, K), ref.inner(Kt, Kt), Kt.sum(), np.trace(K), ref.hsic1(K, K)]
    # sizes of what each sum adds up (its terms in absolute value): a sum of n-long chains and 8-deep trees is within
    # 64 U of that
    size = [want[0], want[1], np.abs(Kt).sum(), np.abs(np.diagonal(K)).sum(),
            (want[1] + np.abs(Kt).sum() ** 2 / ((n - 1) * (n - 2)) + 2 * (np.abs(Kt).sum(axis=1) ** 2).sum() / (n - 2)) / (n * (n - 3))]
    for got, w, sz in zip(S[:5], want, size):
        assert abs(got - float(w)) <= 64 * ref.U * float(sz)
    assert not S[5:8].any() and not S[8 + 21:].any()
    assert np.allclose(S[8:8 + 21], Kt.sum(axis=1).astype(np.float64), rtol=0, atol=64 * ref.U * float(np.abs(K).sum(axis=1).max()))


# ------------------------------------------------------------------------------------------------ pitched layers
def pitched(X, groups, c, pitch, row_stride, pad, lead=0):
    """the layer X [n, groups * c] inside a buffer of ``row_stride`` floats per row, ``lead`` floats in: pads = ``pad``"""
    n = X.shape[0]
    buf = torch.full((lead + n * row_stride + 8,), pad, dtype=torch.float32, device=DEV)
    view = torch.as_strided(buf, (n, 1, groups, pitch), (row_stride, groups * pitch, pitch, 1), lead)
    view[..., :c] = dev(X).view(n, 1, groups, c)
    return engine.PitchedFeatures(view, c), buf


@pytest.mark.parametrize("pad", [float("nan"), 1e30])
@pytest.mark.parametrize("shape", [(4, 38, 48, 201, 0), (1, 5, 8, 9, 0), (3, 8, 12, 40, 4), (260, 4, 8, 2080, 0)])
def test_pitched_layers_have_the_dense_layers_bits(shape, pad):
    """odd row strides (element loads), an aligned one (float4 loads) and one of more than a slab; the pads are poison"""
    groups, c, pitch, rs, lead = shape
    X = features(groups * 100 + c, 13, groups * c)
    dense = engine.device_cka_gram([dev(X)])
    layer, buf = pitched(X, groups, c, pitch, rs, pad, lead)
    got = engine.device_cka_gram([layer])
    assert got.status.tolist() == [0]
    assert same_bits(got.gram, dense.gram) and same_bits(got.sums, dense.sums)
    assert same_bits(layer.dense(), dev(X))


def test_gram_bits_do_not_depend_on_alignment_stride_or_company():
    X = features(3, 37, 2 * SLAB + 8)
    alone = engine.device_cka_gram([dev(X)])                          # float4 loads
    wide = torch.zeros(37, 2 * SLAB + 13, device=DEV)
    wide[:, 1:1 + X.shape[1]] = dev(X)
    shifted = engine.device_cka_gram([wide[:, 1:1 + X.shape[1]]])     # element loads, another row stride
    assert same_bits(alone.gram, shifted.gram) and same_bits(alone.sums, shifted.sums)
    others = [dev(features(50 + k, 37, p)) for k, p in enumerate((1, 5, 64, 300, SLAB + 1, 7, 2, 90))]
    among = engine.device_cka_gram(others[:4] + [dev(X)] + others[4:])  # L = 9
    assert same_bits(alone.gram[0], among.gram[4]) and same_bits(alone.sums[0], among.sums[4])
    least = _hip.load().dt_cka_min_workspace_bytes(37, X.shape[1])
    assert least < _hip.load().dt_cka_workspace_bytes(1, 37, X.shape[1])
    for cap in (least, least + 40000):                                # one slab, then two slabs a turn
        turns = engine.device_cka_gram([dev(X)], workspace_bytes=cap)
        assert same_bits(alone.gram, turns.gram) and same_bits(alone.sums, turns.sums)


# ------------------------------------------------------------------------------------------------ bit contracts
def test_scores_transpose_scale_and_copy_contracts():
    c = cka_cases.case("small")
    a, b = [dev(X) for X in c["a"]], [dev(X) for X in c["b"]]
    ab, ba = engine.device_cka(a, b), engine.device_cka(b, a)
    for k in ("cka", "cka_unbiased"):
        assert same_bits(ab[k], ba[k].t())
    assert same_bits(ab["hsic"], ba["hsic"].transpose(0, 1))
    for scale in (2.0 ** 7, 2.0 ** -5):
        scaled = engine.device_cka([a[0] * scale, a[1], a[2] * scale], [b[0], b[1] * scale])
        for k in ("cka", "cka_unbiased"):
            assert same_bits(ab[k], scaled[k]), (k, scale)
    both = engine.device_cka(a + b, [t.clone() for t in a + b])
    assert both["status_a"].tolist() == [0] * 5
    for k in ("cka", "cka_unbiased"):
        assert (torch.diagonal(both[k]) == 1.0).all(), k
        assert same_bits(both[k], both[k].t())
    self_form = engine.device_cka(a + b)
    for k in ("cka", "cka_unbiased", "hsic"):
        assert same_bits(self_form[k], both[k])
    ga = engine.device_cka_gram(a)                                    # Grams made once, scored twice
    assert same_bits(engine.device_cka(ga, b)["cka_unbiased"], ab["cka_unbiased"])
    assert same_bits(engine.device_cka(b, ga)["cka"], ba["cka"])


def test_one_call_form_has_the_two_step_bits():
    c = cka_cases.case("small")
    lib = _hip.load()

    def side(layers):
        descs, n = engine._cka_layers([dev(X) for X in layers], "a")
        L = len(descs)
        args = [(ctypes.c_void_p * L)(*[d[0].data_ptr() for d in descs]), (ctypes.c_longlong * L)(*[d[1] for d in descs])]
        args += [(ctypes.c_int * L)(*[d[k] for d in descs]) for k in (2, 3, 4)]
        out = [torch.empty(L, n, n, dtype=torch.float64, device=DEV), torch.empty(L, engine.CKA_SUMS, dtype=torch.float64, device=DEV),
               torch.empty(L, dtype=torch.int32, device=DEV)]
        return descs, args + [L] + [_hip.ptr(t) for t in out], out
    n = c["n"]
    ws = torch.empty(lib.dt_cka_workspace_bytes(3, n, 64), dtype=torch.uint8, device=DEV)
    two = engine.device_cka([dev(X) for X in c["a"]], [dev(X) for X in c["b"]])
    (keep_a, args_a, out_a), (keep_b, args_b, out_b) = side(c["a"]), side(c["b"])
    res = [torch.empty(3, 2, dtype=torch.float64, device=DEV), torch.empty(3, 2, dtype=torch.float64, device=DEV),
           torch.empty(3, 2, 2, dtype=torch.float64, device=DEV)]
    _hip.check(lib.dt_cka(*args_a, *args_b, n, *[_hip.ptr(t) for t in res], _hip.ptr(ws), ws.numel(), _hip.stream_ptr()), "dt_cka")
    for got, k in zip(res, ("cka", "cka_unbiased", "hsic")):
        assert same_bits(got, two[k]), k
    own = engine.device_cka([dev(X) for X in c["a"]])
    res = [torch.empty(3, 3, dtype=torch.float64, device=DEV), torch.empty(3, 3, dtype=torch.float64, device=DEV)]
    nothing = [None] * 5 + [0] + [None] * 3
    _hip.check(lib.dt_cka(*args_a, *nothing, n, _hip.ptr(res[0]), _hip.ptr(res[1]), None, _hip.ptr(ws), ws.numel(),
                          _hip.stream_ptr()), "dt_cka")
    assert same_bits(res[0], own["cka"]) and same_bits(res[1], own["cka_unbiased"])
    assert same_bits(out_a[0], engine.device_cka_gram([dev(X) for X in c["a"]]).gram)


# ------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("name", sorted(cka_cases.CASES))
def test_scores_against_the_yardstick_within_the_forward_bound(name):
    c = cka_cases.case(name)
    got = engine.device_cka([dev(X) for X in c["a"]], [dev(X) for X in c["b"]])
    assert got["status_a"].tolist() == list(c["ref"]["status_a"]) and got["status_b"].tolist() == list(c["ref"]["status_b"])
    for k, bound in zip(("cka", "cka_unbiased"), c["bound"]):
        err = np.abs((got[k].cpu().numpy().astype(np.longdouble) - c["ref"][k]).astype(np.float64))
        print(f"scores {name} {k}: worst error / bound {float((err / bound).max()):.3g} (bound {bound.max():.3g})")
        assert (err <= bound).all(), f"{name} {k}: worst error / bound {float((err / bound).max()):.3g}"
    if name in cka_cases.NEAR_ZERO:
        assert abs(got["cka_unbiased"].item()) < 0.1 < 0.5 < got["cka"].item()
    hs = got["hsic"].cpu().numpy()
    Ka, Kb = c["ref"]["grams_a"], c["ref"]["grams_b"]
    for i in range(len(Ka)):
        for j in range(len(Kb)):
            scale = float(np.sqrt(ref.inner(Ka[i], Ka[i]) * ref.inner(Kb[j], Kb[j])))
            assert abs(hs[i, j, 0] - float(ref.inner(Ka[i], Kb[j]))) <= c["bound"][0][i, j] * scale
            self_terms = float(np.sqrt(ref.hsic1(Ka[i], Ka[i]) * ref.hsic1(Kb[j], Kb[j])))
            assert abs(hs[i, j, 1] - float(ref.hsic1(Ka[i], Kb[j]))) <= c["bound"][1][i, j] * self_terms


# ------------------------------------------------------------------------------------------------ status
def test_status_bits_and_untouched_neighbours():
    c = cka_cases.case("small")
    clean = [dev(X) for X in c["a"]]
    want = engine.device_cka(clean, clean)
    Z, _ = ref.nonpositive_self_layer()
    for bad, bit in ((None, engine.CKA_NONFINITE), (np.full((12, 9), 2.5, dtype=np.float32), engine.CKA_ZERO_VARIANCE)):
        if bad is None:
            bad = c["a"][1].copy()
            bad[7, 11] = np.nan
        layers = [clean[0], dev(bad), clean[2]]
        g = engine.device_cka_gram(layers)
        assert g.status.tolist() == [0, bit, 0]
        if bit == engine.CKA_NONFINITE:
            assert torch.isnan(g.gram[1]).all() and torch.isnan(g.sums[1, :5]).all()
        got = engine.device_cka(g, clean)
        for k in ("cka", "cka_unbiased"):
            assert torch.isnan(got[k][1]).all(), (k, bit)
            assert same_bits(got[k][[0, 2]], want[k][[0, 2]]), (k, bit)
        assert same_bits(g.gram[[0, 2]], engine.device_cka_gram(clean).gram[[0, 2]])
    inf = c["a"][0].copy()
    inf[0, 0] = np.inf
    assert engine.device_cka_gram([dev(inf)]).status.tolist() == [engine.CKA_NONFINITE]
    four = [dev(c["a"][2][:4]), dev(Z), dev(c["a"][1][:4])]          # n = 4: the constructed layer of the yardstick
    g = engine.device_cka_gram(four)
    assert g.status.tolist() == [0, engine.CKA_SELF_NOT_POSITIVE, 0] == [ref.status(t.cpu().numpy()) for t in four]
    assert g.sums[1, 4].item() <= 0.0 < g.sums[1, 0].item()
    got, clean4 = engine.device_cka(g), engine.device_cka([four[0], four[2]])
    assert torch.isnan(got["cka_unbiased"][1]).all() and torch.isnan(got["cka_unbiased"][:, 1]).all()
    assert torch.isfinite(got["cka"]).all()
    for k in ("cka", "cka_unbiased"):
        assert same_bits(got[k][[0, 2]][:, [0, 2]], clean4[k])


# ------------------------------------------------------------------------------------------------ U-Net readout
@pytest.mark.parametrize("sf", [0.1, 0.3])
def test_block_features_read_the_layered_forward_and_leave_the_handle_alone(models, sf):
    m = copy.deepcopy(models(sf)).to(DEV).eval()
    h = engine.UNetHandle.for_module(m)
    x = seeded_noise(5, (8, 3, 16, 16)).to(DEV)
    tb = h.time_bias([17], [COND_ONE])
    fused = h.fused_active(16, 16)
    assert fused == (sf == 0.1)
    before = h.forward(x, tb, 1, 8)
    plans = dict(h._plans)
    feats = h.block_features(x, tb, 1, 8)
    got = [f.dense().clone() for f in feats]
    real = [m.dims[0], m.dims[1], m.dims[2], m.dims[3], m.dims[3], m.dims[2], m.dims[1], m.dims[0]]
    assert [f.c for f in feats] == real and [tuple(f.view.shape[:3]) for f in feats] == [
        (8, s, s) for s in (16, 8, 4, 2, 1, 2, 4, 8)]
    if sf == 0.3:
        assert feats[0].c == 38 and feats[0].view.shape[3] == 48
    grams = engine.device_cka_gram(feats)                              # straight from the workspace
    assert same_bits(grams.gram, engine.device_cka_gram(got).gram)
    assert h.fused_active(16, 16) == fused and h._plans == plans and h._head_fusion
    after = h.forward(x, tb, 1, 8)
    assert same_bits(before, after)
    h.set_head_fusion(False)
    try:
        h.forward(x, tb, 1, 8)
        for j, f in enumerate(feats):
            want = h.debug_activation(8, 16, 16, j)[..., :real[j]].reshape(8, -1)
            assert same_bits(got[j], want), engine.BLOCK_NAMES[j]
    finally:
        h.set_head_fusion(True)
    two = h.block_features(x, tb, 1, 8, blocks=(4, 0))
    assert same_bits(two[0].dense(), got[4]) and same_bits(two[1].dense(), got[0])
    with pytest.raises(ValueError):
        h.block_features(x, tb, 1, 8, blocks=(8,))


def test_readme_example_runs_as_written(models):
    """the README's usage block: cka_layers without a condition, and the engine calls it shows"""
    from distillation_trajectories_amd.analysis.metrics import cka_layers
    teacher = copy.deepcopy(models(0.3)).to(DEV).eval()
    student = copy.deepcopy(models(0.1)).to(DEV).eval()
    x, t = seeded_noise(9, (8, 3, 16, 16)).to(DEV), torch.tensor([5])
    r = cka_layers(teacher, student, x, t, cond=None)
    assert r["cka"].shape == r["cka_unbiased"].shape == (8, 8) and r["blocks"] == list(engine.BLOCK_NAMES)
    assert not r["status_a"].any() and not r["status_b"].any()
    assert np.isfinite(r["cka"]).all() and np.isfinite(r["cka_unbiased"]).all() and (r["cka"] <= 1 + 1e-12).all()
    h = engine.UNetHandle.for_module(teacher)
    tb, tb_div = engine.time_bias_rows(h, x.shape[0], t)
    feats = h.block_features(x, tb, 1, tb_div)
    grams = engine.device_cka_gram(feats)
    dense_a, view_nhwc = feats[0].dense().clone(), feats[1].view.clone()
    s = engine.device_cka(grams, [dense_a, engine.PitchedFeatures(view_nhwc, feats[1].c)])
    assert tuple(s["cka"].shape) == (8, 2) and tuple(s["hsic"].shape) == (8, 2, 2)
    assert s["cka"][0, 0].item() == 1.0 and s["cka_unbiased"][1, 1].item() == 1.0
    own = engine.device_cka(grams)
    assert same_bits(own["cka"], torch.from_numpy(cka_layers(teacher, teacher, x, t)["cka"]))


# ------------------------------------------------------------------------------------------------ the sweep
def test_cka_sweep_tiny(models, tmp_path):
    from distillation_trajectories_amd.analysis.trajectory_engine import sample_grid
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.synthetic import noise_table
    cfg = Config()
    cfg.image_size, cfg.timesteps = 16, 4
    T, S = 4, 6
    teacher = copy.deepcopy(models(0.3)).to(DEV).eval()
    students = [copy.deepcopy(models(0.3)).to(DEV).eval(), copy.deepcopy(models(0.1)).to(DEV).eval()]
    res = representation.cka_sweep(teacher, students, cfg, S, every=2, output_dir=str(tmp_path))
    assert res["states"].tolist() == [0, 2, 3] and res["timesteps"].tolist() == [3, 1, 0]
    assert res["cka"].shape == res["cka_unbiased"].shape == (2, 3, 8, 8)
    assert res["teacher_self"].shape == res["teacher_self_unbiased"].shape == (3, 8, 8)
    assert res["status"].shape == (3, 3, 8) and not res["status"].any()
    assert list(res["blocks"]) == list(engine.BLOCK_NAMES)
    for k in ("teacher_self", "teacher_self_unbiased"):
        for own in res[k]:
            assert (np.diagonal(own) == 1.0).all(), k
            assert np.array_equal(own.view(np.int64), own.T.copy().view(np.int64)), k
    assert np.array_equal(res["cka"][0].view(np.int64), res["teacher_self"].view(np.int64))          # the weight copy
    assert np.array_equal(res["cka_unbiased"][0].view(np.int64), res["teacher_self_unbiased"].view(np.int64))
    assert np.isfinite(res["cka"][1]).all() and (np.abs(res["cka"][1]) <= 1 + 1e-12).all()
    for j in range(2):
        with np.load(os.path.join(str(tmp_path), f"cka_student_{j}.npz")) as f:
            assert sorted(f.files) == sorted(["cka", "cka_unbiased", "teacher_self", "teacher_self_unbiased", "status", "states",
                                              "timesteps", "blocks"])
            assert np.array_equal(f["cka"], res["cka"][j]) and f["status"].shape == (2, 3, 8)
    table = noise_table(42, S + T - 1, (1, 3, 16, 16)).reshape(S + T - 1, -1).to(DEV)
    states = sample_grid(engine.UNetHandle.for_module(teacher), table, 0, S, T, [None], 16, 16)[None]
    one = representation.cka_layers(teacher, students[1], states[2].reshape(S, 3, 16, 16), torch.tensor([1]),
                                    cond=torch.ones(1, 1, device=DEV))
    assert np.array_equal(one["cka"].view(np.int64), res["cka"][1][1].view(np.int64))
    assert np.array_equal(one["cka_unbiased"].view(np.int64), res["cka_unbiased"][1][1].view(np.int64))
    assert one["blocks"] == list(engine.BLOCK_NAMES) and not one["status_a"].any()
