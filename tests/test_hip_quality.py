"""GPU: the device sample-quality scores (include/dt_hip_quality.h, csrc/dt_quality.hip, engine.device_quality,
analysis/metrics/sample_quality.py) against the float64 yardstick quality_ref64: the listed shapes, identical and duplicated
sets (the strict-< tie contract), KID subsets, the status word, bit-identity across batching, sharing, strides, calls and
workspace contents, the stage events, and the drivers on real pipeline features.

Bounds (quality_ref64's docstring derives them; u = 2^-53): a squared radius within 4 (D + 4) u max |row|^2 of its set, KID
within 4 (3 (D + 2) + n_a + n_b) u S_kappa; counts exactly, after the yardstick alone has shown that every comparison that
is not an exact tie between bitwise-equal rows is decided by at least 100 bounds.  Every case prints its deviations, in
units of its bound, before it asserts."""
import numpy as np
import pytest
import torch

import inception_ref as iref
import quality_ref64 as q
from distillation_trajectories_amd import engine, inception
from distillation_trajectories_amd.analysis.metrics import fid_score, guidance_quality_sweep, quality_sweep, sample_quality

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
MIN_GAP = 100.0
FIELDS = ("kid", "kid_subsets", "counts", "precision", "recall", "density", "coverage", "status")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _same(r1, r2, fields=FIELDS + ("radii_a", "radii_b"), rows=slice(None)):
    """whether the listed outputs have the same bits (NaN included)"""
    return all(r1[f].cpu().numpy().tobytes() == r2[f][rows].cpu().numpy().tobytes() for f in fields)


def _check(r, p, a, b, k, ref, what):
    """problem p of the result r (taken with radii) against the yardstick of (a, b, k)"""
    n_a, n_b = len(a), len(b)
    assert ref["min_gap"] >= MIN_GAP, (what, ref["min_gap"])
    counts = r["counts"][p].cpu().numpy()
    ba, bb = q.radius_bounds(a, b)
    da = np.abs(r["radii_a"][p].cpu().numpy() - ref["radii_a"]).max() / ba if ba else 0.0
    db = np.abs(r["radii_b"][p].cpu().numpy() - ref["radii_b"]).max() / bb if bb else 0.0
    kid = float(r["kid"][p])
    dk = abs(kid - ref["kid"]) / ref["kid_tol"]
    print(f"{what}: counts {counts.tolist()} ref {ref['counts'].tolist()}  radii off by {da:.3g} / {db:.3g} bounds  kid "
          f"{kid!r} ref {ref['kid']!r} off by {dk:.3g} bounds  (comparison gap {ref['min_gap']:.3g} bounds)")
    assert int(r["status"][p]) == 0
    assert counts.tolist() == ref["counts"].tolist(), what
    assert da <= 1.0 and db <= 1.0, (what, da, db)
    if not ba:
        assert (r["radii_a"][p] == 0.0).all()
    if not bb:
        assert (r["radii_b"][p] == 0.0).all()
    assert np.isfinite(kid) and dk <= 1.0, (what, dk)
    c = counts.astype(np.float64)
    for name, want in (("precision", c[0] / n_b), ("recall", c[1] / n_a), ("density", c[2] / (k * n_b)),
                       ("coverage", c[3] / n_a)):
        assert float(r[name][p]) == want, (what, name)


@pytest.mark.parametrize("name", list(q.SHAPES))
def test_shapes_match_ref64(name):
    n_a, n_b, P, D, k = q.SHAPES[name]
    a, bs, k, refs = q.shape_case(name)
    ta = _dev(a)                                                              # 2-D: shared by all P problems
    tb = _dev(np.stack(bs)) if P > 1 else _dev(bs[0])
    r = engine.device_quality(ta, tb, k=k, radii=True)
    assert r["kid"].shape == (P,) and r["kid_subsets"].shape == (P, 0) and r["counts"].shape == (P, 4)
    assert r["radii_a"].shape == (P, n_a) and r["radii_b"].shape == (P, n_b) and r["status"].shape == (P,)
    assert r["kid"].dtype == torch.float64 and r["counts"].dtype == torch.int64 and r["precision"].dtype == torch.float64
    for p in range(P):
        _check(r, p, a, bs[p], k, refs[p], (name, p))
    assert "radii_a" not in engine.device_quality(ta, tb, k=k)
    if n_a < 2048:                              # the sets the other way round: precision and recall swap, KID stays
        r2 = engine.device_quality(tb, ta, k=k, radii=True)
        for p in range(P):
            c, c2 = r["counts"][p].tolist(), r2["counts"][p].tolist()
            assert (c2[0], c2[1]) == (c[1], c[0]), (name, p, c, c2)
            assert abs(float(r2["kid"][p]) - refs[p]["kid"]) <= refs[p]["kid_tol"], (name, p)
            assert torch.equal(r2["radii_a"][p], r["radii_b"][p]) and torch.equal(r2["radii_b"][p], r["radii_a"][p])


def test_identical_and_duplicated_sets():
    # B a bitwise copy of A: each a_i's k-th neighbour sits exactly on the radius and is not counted, so density is 1
    a, b, k, ref = q.special_case("identical")
    n = len(a)
    r = engine.device_quality(_dev(a), _dev(b), k=k, radii=True)
    _check(r, 0, a, b, k, ref, "identical")
    assert r["counts"][0].tolist() == [n, n, n * k, n]
    assert [float(r[f][0]) for f in ("precision", "recall", "density", "coverage")] == [1.0, 1.0, 1.0, 1.0]
    assert torch.equal(r["radii_a"], r["radii_b"])
    for name in ("copies", "x4", "constant_a", "constant_b"):
        a, b, k, ref = q.special_case(name)
        r = engine.device_quality(_dev(a), _dev(b), k=k, radii=True)
        _check(r, 0, a, b, k, ref, name)
        if name.startswith("constant"):                     # radii 0, nothing is < 0, no error
            assert (r["radii_a" if name == "constant_a" else "radii_b"] == 0.0).all()
            assert r["counts"][0].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("n_a,n_b,S,m", [(50, 50, 7, 20), (130, 70, 3, 70)])
def test_subsets(n_a, n_b, S, m):
    D = 2048
    a, b = q.feature_pair(50 + n_a, n_a, n_b, D, "shift", 1)
    ia, ib = sample_quality.kid_subset_tables(n_a, n_b, S, m, seed=n_a)
    ta, tb = _dev(a), _dev(b)
    r = engine.device_quality(ta, tb, k=5, subsets=(ia, ib))
    assert r["kid_subsets"].shape == (1, S) and _same(engine.device_quality(ta, tb, k=5), r, ("kid", "counts"))
    assert _same(engine.device_quality(ta, tb, k=5, subsets=(torch.from_numpy(ia).to(DEV), torch.from_numpy(ib))), r, FIELDS)
    gathered = engine.device_quality(_dev(a[ia]), _dev(b[ib]), k=1)           # the S subsets as S full-set problems
    for s in range(S):
        want, s_kappa = q.kid_ref64(a[ia[s]], b[ib[s]])
        tol = q.kid_tolerance(m, m, D, s_kappa)
        got = float(r["kid_subsets"][0, s])
        print(f"subset {s}: {got!r} ref {want!r} off by {abs(got - want) / tol:.3g} bounds, from the gathered rows by "
              f"{abs(got - float(gathered['kid'][s])) / tol:.3g}")
        assert abs(got - want) <= tol and abs(got - float(gathered["kid"][s])) <= tol, s
    res = sample_quality.calculate_kid_device(a, b, num_subsets=S, subset_size=m, seed=n_a)
    sub = r["kid_subsets"][0].cpu().numpy()
    assert res == {"kid": float(r["kid"][0]), "kid_mean": float(sub.mean()), "kid_std": float(sub.std())}
    rep, out = ia.copy(), ib.copy()
    rep[1, 4] = rep[1, 0]
    out[2, 2] = n_b
    with pytest.raises(ValueError, match="repeats"):
        engine.device_quality(ta, tb, subsets=(rep, ib))
    with pytest.raises(ValueError, match="outside"):
        engine.device_quality(ta, tb, subsets=(ia, out))


def test_status_words_isolate_bad_problems():
    D, P, k = 256, 5, 3
    a = q.feature_pair(12, 30, 24, D)[0]
    bs = np.stack([q.feature_pair(12, 30, 24, D, "shift", p)[1] for p in range(P)])
    ta, tb = _dev(a), _dev(bs)
    sub = sample_quality.kid_subset_tables(30, 24, 2, 10)
    clean = engine.device_quality(ta, tb, k=k, subsets=sub, radii=True)
    assert clean["status"].cpu().tolist() == [0] * P

    def check(r, bad):
        assert r["status"].cpu().tolist() == [int(p in bad) for p in range(P)]
        for p in range(P):
            if p in bad:
                for f in ("kid", "precision", "recall", "density", "coverage"):
                    assert torch.isnan(r[f][p]), (p, f)
                for f in ("kid_subsets", "radii_a", "radii_b"):
                    assert torch.isnan(r[f][p]).all(), (p, f)
                assert r["counts"][p].tolist() == [-1] * 4
            else:
                one = {f: v[p:p + 1] for f, v in r.items()}
                assert _same(one, clean, rows=slice(p, p + 1)), p

    bad = tb.clone()
    bad[1, 7, 100] = float("nan")
    bad[2, 23, 255] = float("inf")
    bad[4, 0, 0] = float("-inf")
    check(engine.device_quality(ta, bad, k=k, subsets=sub, radii=True), (1, 2, 4))
    ab = ta.unsqueeze(0).repeat(P, 1, 1)                       # a NaN in set a of one problem only
    ab[3, 29, 1] = float("nan")
    check(engine.device_quality(ab, tb, k=k, subsets=sub, radii=True), (3,))
    assert np.isnan(sample_quality.calculate_kid_device(ab[3], tb[3])["kid"])
    assert all(np.isnan(v) for v in sample_quality.calculate_prdc_device(ab[3], tb[3], k=k).values())


@pytest.mark.parametrize("n_a,n_b", [(50, 50), (130, 70)])
def test_bits_do_not_depend_on_batch_sharing_strides_calls_or_workspace(n_a, n_b):
    D, P, k = 2048, 11, 5
    a = _dev(q.feature_pair(21, n_a, n_b, D)[0])
    bs = _dev(np.stack([q.feature_pair(21, n_a, n_b, D, q.MODES[p % 4], p // 4)[1] for p in range(P)]))
    sub = sample_quality.kid_subset_tables(n_a, n_b, 3, 20)
    kw = dict(k=k, subsets=sub, radii=True)
    big = engine.device_quality(a, bs, **kw)                                   # teacher shared
    assert len({tuple(c) for c in big["counts"].tolist()}) > 3
    again = engine.device_quality(a, bs, **kw)
    copied = engine.device_quality(a.unsqueeze(0).repeat(P, 1, 1), bs, **kw)   # teacher copied P times
    expanded = engine.device_quality(a.unsqueeze(0).expand(P, n_a, D), bs, **kw)     # a stride-0 view
    assert _same(again, big) and _same(copied, big) and _same(expanded, big)
    for p in (0, 4, 10):
        assert _same(engine.device_quality(a, bs[p], **kw), big, rows=slice(p, p + 1)), p
    # non-contiguous views: rows of a wider tensor (row stride D + 8) and every other problem of the batch
    wide_a = torch.zeros(n_a, D + 8, device=DEV)
    wide_a[:, :D] = a
    wide_b = torch.full((P, n_b + 3, D + 8), float("nan"), device=DEV)
    wide_b[:, 1:n_b + 1, 4:D + 4] = bs
    va, vb = wide_a[:, :D], wide_b[:, 1:n_b + 1, 4:D + 4]
    assert not va.is_contiguous() and not vb.is_contiguous()
    assert _same(engine.device_quality(va, vb, **kw), big)
    assert _same(engine.device_quality(a, bs[::2], **kw), big, rows=slice(None, None, 2))
    # a poisoned workspace, and a short one
    nbytes = engine._hip.load().dt_quality_workspace_bytes(P, n_a, n_b, D)
    ws = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    assert _same(engine.device_quality(a, bs, workspace=ws, **kw), big)
    with pytest.raises(ValueError, match="workspace"):
        engine.device_quality(a, bs, workspace=ws[:nbytes - 8], **kw)
    assert _same(engine.device_quality(a, bs, **kw), big)


def test_events_bracket_the_stages():
    a, b = (_dev(x) for x in q.feature_pair(41, 50, 50, 2048))
    plain = engine.device_quality(a, b, radii=True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(engine.QUALITY_EVENTS)]
    timed = engine.device_quality(a, b, radii=True, events=ev)
    torch.cuda.synchronize()
    assert all(ev[i].elapsed_time(ev[i + 1]) >= 0.0 for i in range(engine.QUALITY_EVENTS - 1))
    assert ev[0].elapsed_time(ev[-1]) > 0.0
    assert _same(plain, timed)
    with pytest.raises(ValueError, match="events"):
        engine.device_quality(a, b, events=ev[:4])


# ---------------------------------------------------------------------- the drivers on real pipeline features
N_SAMPLES, K_DRIVERS = 6, 2


def _images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tanh(1.5 * torch.randn(n, 3, h, w, generator=g))


@pytest.fixture(scope="module")
def weights():
    """float32 synthetic Inception weights, BatchNorm statistics calibrated so that no layer is dead"""
    sd = iref.random_state_dict(inception.key_table(), seed=11)
    iref.calibrate(sd, _images(4, 32, 32, seed=12).double(), 0.5, 0.5)
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}


def _diffusion_models(n_students=1):
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model
    cfg = Config()
    cfg.image_size, cfg.timesteps, cfg.num_samples = 16, 6, N_SAMPLES
    students = [make_model(DiffusionUNet, cfg, sf).to(DEV) for sf in (0.05, 0.1, 0.15)[:n_students]]
    return cfg, make_model(DiffusionUNet, cfg, 0.2).to(DEV), students


def _pipeline_features(model, cfg, n, inception_model):
    samples = fid_score.generate_samples(model, cfg, n, DEV)
    return fid_score.extract_features(samples, inception_model, batch_size=32, in_scale=0.5, in_shift=0.5)


def test_calculate_kid_and_prdc_device_on_pipeline_features(weights):
    cfg, teacher, (student,) = _diffusion_models()
    m = fid_score.InceptionModel(DEV, weights=weights)
    torch.manual_seed(31)
    tf, sf = _pipeline_features(teacher, cfg, N_SAMPLES, m), _pipeline_features(student, cfg, N_SAMPLES, m)
    a, b, k = tf.cpu().numpy(), sf.cpu().numpy(), K_DRIVERS
    ref = q.quality_ref64(a, b, k)
    kid = sample_quality.calculate_kid_device(tf, sf)
    prdc = sample_quality.calculate_prdc_device(tf, sf, k=k)
    print(f"pipeline features: kid {kid['kid']!r} ref {ref['kid']!r} off by {abs(kid['kid'] - ref['kid']) / ref['kid_tol']:.3g} "
          f"bounds; prdc {prdc} ref counts {ref['counts'].tolist()} (comparison gap {ref['min_gap']:.3g} bounds)")
    assert set(kid) == {"kid", "kid_mean", "kid_std"} and all(isinstance(v, float) for v in kid.values())
    assert np.isnan(kid["kid_mean"]) and np.isnan(kid["kid_std"])
    assert abs(kid["kid"] - ref["kid"]) <= ref["kid_tol"]
    assert ref["min_gap"] >= MIN_GAP
    c = ref["counts"].astype(np.float64)
    n = float(N_SAMPLES)
    assert prdc == {"precision": c[0] / n, "recall": c[1] / n, "density": c[2] / (k * n), "coverage": c[3] / n}
    assert all(isinstance(v, float) for v in prdc.values())
    assert sample_quality.calculate_kid_device(a, sf.cpu())["kid"] == kid["kid"]                # host inputs are uploaded
    assert sample_quality.calculate_prdc_device(a, b, k=k) == prdc
    with_subsets = sample_quality.calculate_kid_device(tf, sf, num_subsets=4, subset_size=4, seed=1)
    ia, ib = sample_quality.kid_subset_tables(N_SAMPLES, N_SAMPLES, 4, 4, seed=1)
    sub = [q.kid_ref64(a[ia[s]], b[ib[s]])[0] for s in range(4)]
    assert with_subsets["kid"] == kid["kid"]
    assert abs(with_subsets["kid_mean"] - np.mean(sub)) <= ref["kid_tol"] and abs(with_subsets["kid_std"] - np.std(sub)) <= ref["kid_tol"]


def test_quality_sweep_equals_separate_calls(weights):
    cfg, teacher, students = _diffusion_models(n_students=3)
    k = K_DRIVERS
    torch.manual_seed(77)
    res = quality_sweep(teacher, students, cfg, N_SAMPLES, weights=weights, k=k, num_subsets=2, subset_size=4, seed=5)
    torch.manual_seed(77)
    fid = fid_score.fid_sweep(teacher, students, cfg, N_SAMPLES, weights=weights)
    assert res["fid"].tobytes() == fid["fid"].tobytes() and res["fid"].shape == (3,)
    assert set(res) == {"fid", "kid", "kid_subsets", "precision", "recall", "density", "coverage", "counts", "status"}
    assert all(isinstance(v, np.ndarray) for v in res.values()) and res["kid_subsets"].shape == (3, 2)
    assert res["counts"].shape == (3, 4) and res["status"].tolist() == [0, 0, 0]
    m = fid_score.InceptionModel(DEV, weights=weights)
    torch.manual_seed(77)
    tf = _pipeline_features(teacher, cfg, N_SAMPLES, m)
    sub = sample_quality.kid_subset_tables(N_SAMPLES, N_SAMPLES, 2, 4, seed=5)
    for i, s in enumerate(students):
        sf = _pipeline_features(s, cfg, N_SAMPLES, m)
        one = engine.device_quality(tf, sf, k=k, subsets=sub)
        for f in FIELDS:
            assert one[f][0].cpu().numpy().tobytes() == res[f][i].tobytes(), (i, f)
        ref = q.quality_ref64(tf.cpu().numpy(), sf.cpu().numpy(), k)
        assert abs(res["kid"][i] - ref["kid"]) <= ref["kid_tol"], i
        if ref["min_gap"] >= MIN_GAP:
            assert res["counts"][i].tolist() == ref["counts"].tolist(), i
    assert len(set(res["kid"].tolist())) == 3


def test_guidance_quality_sweep_equals_calls_by_hand(weights):
    from distillation_trajectories_amd.analysis.trajectory_engine import sample_grid
    from distillation_trajectories_amd.synthetic import noise_table
    cfg, teacher, students = _diffusion_models(n_students=2)
    scales, k, S = (1.0, 3.0), K_DRIVERS, N_SAMPLES
    res = guidance_quality_sweep(teacher, students, cfg, scales, S, weights=weights, k=k)
    assert set(res) == {"fid", "kid", "kid_subsets", "precision", "recall", "density", "coverage", "counts", "status"}
    assert res["kid"].shape == (2, 2) and res["counts"].shape == (2, 2, 4) and res["kid_subsets"].shape == (2, 2, 0)
    assert (res["status"] == 0).all()
    C, H, T = cfg.channels, cfg.image_size, cfg.timesteps
    m = fid_score.InceptionModel(DEV, weights=weights)
    table = noise_table(42, S + T - 1, (1, C, H, H)).reshape(S + T - 1, -1).to(DEV)

    def features(model):
        grid = sample_grid(engine.UNetHandle.for_module(model), table, 0, S, T, list(scales), H, H)
        return [fid_score.extract_features(grid[gs][T].reshape(S, C, H, H).contiguous(), m, batch_size=32, in_scale=0.5,
                                           in_shift=0.5) for gs in scales]

    tf = features(teacher)
    for i, s in enumerate(students):
        sf = features(s)
        for j in range(len(scales)):
            one = engine.device_quality(tf[j], sf[j], k=k)
            for f in FIELDS:
                assert one[f][0].cpu().numpy().tobytes() == res[f][i, j].tobytes(), (i, j, f)
            assert float(engine.device_fid(tf[j], sf[j])["fid"][0]) == res["fid"][i, j]
    assert len(set(res["kid"].ravel().tolist())) == 4
