"""GPU: the device Fréchet distance (include/dt_hip_fid.h, csrc/dt_fid.hip, engine.device_fid) against the float64
yardstick fid_ref64 (numpy SVD of the centred float64 cross product): the listed shapes, degenerate inputs, the status word,
bit-identity across batching, sharing, strides, calls and workspace contents, and the drivers on real pipeline features.

Bounds (s = tr S_a + tr S_b from the yardstick): fid and the cross term within 1e-6 s -- the bound the committed host
formula is held to against the same yardstick in tests/test_fid_host.py; |mu_a - mu_b|^2 and the traces within 1e-9
relative, the project's standing bound for fp64 outputs.  Every case prints its deviation before it asserts."""
import os
import subprocess

import numpy as np
import pytest
import torch

import inception_ref as iref
from distillation_trajectories_amd import engine, inception
from distillation_trajectories_amd.analysis.metrics import fid_score
from fid_ref64 import feature_like, fid_ref64

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
FID_TOL = 1e-6
PART_TOL = 1e-9


def _five(r, p=0):
    """the five doubles of problem p as one host array (fid, then the four parts)"""
    return np.concatenate([r["fid"][p:p + 1].cpu().numpy(), r["parts"][p].cpu().numpy()])


def _same_bits(x, y):
    return x.tobytes() == y.tobytes()


def _check(five, a, b, what):
    ref = fid_ref64(a, b)
    s = ref["scale"]
    dev_fid, dev_cross = abs(five[0] - ref["fid"]) / s, abs(five[4] - ref["parts"][3]) / s
    rel = [abs(five[1 + i] - ref["parts"][i]) / max(abs(ref["parts"][i]), 1e-300) for i in range(3)]
    print(f"{what}: fid {five[0]!r} ref {ref['fid']!r}  |d fid|/s {dev_fid:.3g}  |d cross|/s {dev_cross:.3g}  "
          f"parts rel {max(rel):.3g}")
    assert np.all(np.isfinite(five)), what
    assert dev_fid <= FID_TOL, (what, dev_fid)
    assert dev_cross <= FID_TOL, (what, dev_cross)
    for i, name in enumerate(("dmu2", "tr_a", "tr_b")):
        assert rel[i] <= PART_TOL, (what, name, rel[i])
    return ref


def test_fid_entry_host_code_clean_under_asan_and_ubsan():
    """tests/host_sanitize/fid_driver.cpp (every entry of include/dt_hip_fid.h) under host ASan / UBSan."""
    from distillation_trajectories_amd.csrc.build import FID_SAN_DRIVER, build_fid_sanitizer_driver
    if not os.path.exists(FID_SAN_DRIVER):
        build_fid_sanitizer_driver()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([FID_SAN_DRIVER], capture_output=True, text=True, env=env, timeout=300)
    report = r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, report
    assert r.returncode == 0 and "fid driver ok" in r.stdout, report


@pytest.mark.parametrize("shape", [
    dict(n_a=50, n_b=50, P=1, D=2048),           # the reference's default of 50 samples
    dict(n_a=50, n_b=50, P=11, D=2048),          # one teacher set shared by 11 students
    dict(n_a=8, n_b=50, P=3, D=2048),
    dict(n_a=300, n_b=257, P=2, D=2048),         # M^T M: the smaller side is b's
    dict(n_a=2, n_b=50, P=1, D=2048),            # a single degree of freedom
    dict(n_a=2048, n_b=2048, P=1, D=2048),       # the largest side
    dict(n_a=1200, n_b=1000, P=1, D=2048),
    dict(n_a=300, n_b=257, P=2, D=64),           # more samples than features: rank capped by D
    dict(n_a=65, n_b=64, P=2, D=80),             # M^T M, one row of a into the second tile
    dict(n_a=64, n_b=65, P=2, D=80),             # M M^T, one row of b into the second tile
    dict(n_a=129, n_b=63, P=1, D=36),            # three tile rows of a; the last stage holds one quad
], ids=["50x50", "50x50_P11_shared", "8x50_P3", "300x257_P2", "2x50", "2048x2048", "1200x1000", "D64_300x257_P2",
        "D80_65x64_P2", "D80_64x65_P2", "D36_129x63"])
def test_shapes_match_ref64(shape):
    n_a, n_b, P, D = shape["n_a"], shape["n_b"], shape["P"], shape["D"]
    a = feature_like(1000 + n_a, n_a, D)
    bs = [feature_like(2000 + n_b + p, n_b, D, shift=0.01 * (p + 1), spread=0.15 + 0.02 * p) for p in range(P)]
    ta = torch.from_numpy(a).to(DEV)                                       # 2-D: shared by all P problems
    tb = torch.from_numpy(np.stack(bs)).to(DEV) if P > 1 else torch.from_numpy(bs[0]).to(DEV)
    r = engine.device_fid(ta, tb)
    assert r["fid"].shape == (P,) and r["parts"].shape == (P, 4) and r["status"].shape == (P,)
    assert r["fid"].dtype == torch.float64 and r["parts"].dtype == torch.float64
    assert r["status"].cpu().tolist() == [0] * P
    for p in range(P):
        five = _five(r, p)
        _check(five, a, bs[p], (shape, p))
        assert five[0] == five[1] + five[2] + five[3] - 2.0 * five[4]
    if P > 1:                                      # the sets the other way round: fid is symmetric, the traces swap
        r2 = engine.device_fid(tb, ta)
        for p in range(P):
            five = _five(r2, p)
            _check(five, bs[p], a, (shape, p, "swapped"))


def test_degenerate_inputs():
    D = 2048
    a = feature_like(5, 60, D)
    # both sets identical: 0 within rounding, possibly negative, not clamped
    five = _five(engine.device_fid(torch.from_numpy(a).to(DEV), torch.from_numpy(a.copy()).to(DEV)))
    ref = _check(five, a, a, "identical")
    print(f"identical sets: fid {five[0]!r} (s = {ref['scale']!r})")
    assert abs(five[0]) <= FID_TOL * ref["scale"] and five[1] == 0.0 and five[2] == five[3]
    # features in a 20-dimensional subspace: 280 and 237 eigenvalues that are 0 up to rounding
    lo_a, lo_b = feature_like(6, 300, D, rank=20), feature_like(7, 257, D, rank=20, shift=0.01)
    _check(_five(engine.device_fid(torch.from_numpy(lo_a).to(DEV), torch.from_numpy(lo_b).to(DEV))), lo_a, lo_b, "rank 20")
    same_space = feature_like(6, 300, D, rank=20)[:257] * np.float32(1.0)    # and the same subspace on both sides
    _check(_five(engine.device_fid(torch.from_numpy(lo_a).to(DEV), torch.from_numpy(same_space).to(DEV))), lo_a, same_space,
           "rank 20, one subspace")
    # every row four times
    du_a, du_b = np.repeat(a, 4, axis=0), np.repeat(feature_like(8, 50, D, shift=0.02), 4, axis=0)
    _check(_five(engine.device_fid(torch.from_numpy(du_a).to(DEV), torch.from_numpy(du_b).to(DEV))), du_a, du_b, "duplicated x4")
    # one constant set: no error, its trace and the cross term are exactly 0
    const = np.full((40, D), 0.37, np.float32)
    for x, y, tr in ((const, a, 2), (a, const, 3)):
        r = engine.device_fid(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
        five = _five(r)
        _check(five, x, y, "constant set")
        assert r["status"].cpu().tolist() == [0] and five[tr] == 0.0 and five[4] == 0.0
    r = engine.device_fid(torch.full((40, D), 0.25, device=DEV), torch.full((9, D), 0.75, device=DEV))
    assert np.array_equal(_five(r), [0.25 * D, 0.25 * D, 0.0, 0.0, 0.0])


def test_status_words_isolate_bad_problems():
    D, P = 256, 5
    a = feature_like(11, 30, D)
    bs = np.stack([feature_like(12 + p, 24, D, shift=0.01) for p in range(P)])
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(bs).to(DEV)
    clean = engine.device_fid(ta, tb)
    assert clean["status"].cpu().tolist() == [0] * P
    bad = tb.clone()
    bad[1, 7, 100] = float("nan")
    bad[2, 23, 255] = float("inf")
    bad[4, 0, 0] = float("-inf")
    r = engine.device_fid(ta, bad)
    assert r["status"].cpu().tolist() == [0, 1, 1, 0, 1]
    for p in (1, 2, 4):
        assert np.all(np.isnan(_five(r, p))), p
    for p in (0, 3):
        assert _same_bits(_five(r, p), _five(clean, p)), p
    # a NaN in set a of one problem only
    ab = ta.unsqueeze(0).repeat(P, 1, 1)
    ab[3, 29, 1] = float("nan")
    r = engine.device_fid(ab, tb)
    assert r["status"].cpu().tolist() == [0, 0, 0, 1, 0]
    assert np.all(np.isnan(_five(r, 3)))
    for p in (0, 1, 2, 4):
        assert _same_bits(_five(r, p), _five(clean, p)), p
    assert np.isnan(fid_score.calculate_fid_device(ab[3], tb[3]))


@pytest.mark.parametrize("n_a,n_b", [(50, 50), (130, 70)])
def test_bits_do_not_depend_on_batch_sharing_strides_calls_or_workspace(n_a, n_b):
    D, P = 2048, 11
    a = torch.from_numpy(feature_like(21, n_a, D)).to(DEV)
    bs = torch.from_numpy(np.stack([feature_like(30 + p, n_b, D, shift=0.01 * p) for p in range(P)])).to(DEV)
    big = engine.device_fid(a, bs)                                             # teacher shared
    again = engine.device_fid(a, bs)
    copied = engine.device_fid(a.unsqueeze(0).repeat(P, 1, 1), bs)             # teacher copied P times
    expanded = engine.device_fid(a.unsqueeze(0).expand(P, n_a, D), bs)         # a stride-0 view
    for f in ("fid", "parts", "status"):
        assert torch.equal(big[f], again[f]) and torch.equal(big[f], copied[f]) and torch.equal(big[f], expanded[f]), f
    for p in (0, 4, 10):
        alone = engine.device_fid(a, bs[p])
        assert _same_bits(_five(alone), _five(big, p)), p
    # non-contiguous views: rows of a wider tensor (row stride D + 8) and every other problem of the batch
    wide_a = torch.zeros(n_a, D + 8, device=DEV)
    wide_a[:, :D] = a
    wide_b = torch.full((P, n_b + 3, D + 8), float("nan"), device=DEV)
    wide_b[:, 1:n_b + 1, 4:D + 4] = bs
    va, vb = wide_a[:, :D], wide_b[:, 1:n_b + 1, 4:D + 4]
    assert not va.is_contiguous() and not vb.is_contiguous()
    view = engine.device_fid(va, vb)
    for f in ("fid", "parts", "status"):
        assert torch.equal(view[f], big[f]), f
    half = engine.device_fid(a, bs[::2])
    assert torch.equal(half["fid"], big["fid"][::2]) and torch.equal(half["parts"], big["parts"][::2])
    # a poisoned workspace
    nbytes = engine._hip.load().dt_fid_workspace_bytes(P, n_a, n_b, D)
    ws = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    poisoned = engine.device_fid(a, bs, workspace=ws)
    for f in ("fid", "parts", "status"):
        assert torch.equal(poisoned[f], big[f]), f
    with pytest.raises(ValueError, match="workspace"):
        engine.device_fid(a, bs, workspace=ws[:nbytes - 8])


def test_events_bracket_the_stages():
    a = torch.from_numpy(feature_like(41, 50, 2048)).to(DEV)
    b = torch.from_numpy(feature_like(42, 50, 2048)).to(DEV)
    plain = engine.device_fid(a, b)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(engine.FID_EVENTS)]
    timed = engine.device_fid(a, b, events=ev)
    torch.cuda.synchronize()
    assert all(ev[i].elapsed_time(ev[i + 1]) >= 0.0 for i in range(engine.FID_EVENTS - 1))
    assert ev[0].elapsed_time(ev[-1]) > 0.0
    assert _same_bits(_five(plain), _five(timed))


# ---------------------------------------------------------------------- the drivers on real pipeline features
def _images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tanh(1.5 * torch.randn(n, 3, h, w, generator=g))


@pytest.fixture(scope="module")
def weights():
    """float32 synthetic Inception weights, BatchNorm statistics calibrated so that no layer is dead"""
    sd = iref.random_state_dict(inception.key_table(), seed=11)
    iref.calibrate(sd, _images(4, 32, 32, seed=12).double(), 0.5, 0.5)
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}


def _diffusion_models(n_students=1, num_samples=5):
    from distillation_trajectories_amd.config import Config
    from distillation_trajectories_amd.models import DiffusionUNet
    from distillation_trajectories_amd.synthetic import make_model
    cfg = Config()
    cfg.image_size, cfg.timesteps, cfg.num_samples = 16, 6, num_samples
    students = [make_model(DiffusionUNet, cfg, sf).to(DEV) for sf in (0.05, 0.1, 0.15)[:n_students]]
    return cfg, make_model(DiffusionUNet, cfg, 0.2).to(DEV), students


def _pipeline_features(model, cfg, n, inception_model):
    samples = fid_score.generate_samples(model, cfg, n, DEV)
    return fid_score.extract_features(samples, inception_model, batch_size=32, in_scale=0.5, in_shift=0.5)


def test_calculate_fid_device_against_the_host_formula_on_pipeline_features(weights):
    """Teacher sf 0.2 against student sf 0.05, 5 samples each at 16 x 16, T = 6, as test_hip_inception's driver test builds
    them.  Measured on an MI355X: |device - yardstick| = 3.1e-9 s, |device - host| = 8.1e-7 s (s = 2341): nearly all of the
    second figure is the host formula's own distance from the yardstick (scipy's sqrtm of a rank-4 2048 x 2048 product),
    so this comparison holds with little margin and the yardstick one with a wide one."""
    cfg, teacher, (student,) = _diffusion_models()
    m = fid_score.InceptionModel(DEV, weights=weights)
    torch.manual_seed(31)
    tf, sf = _pipeline_features(teacher, cfg, 5, m), _pipeline_features(student, cfg, 5, m)
    got = fid_score.calculate_fid_device(tf, sf)
    assert isinstance(got, float)
    host = fid_score.calculate_fid(tf.cpu().numpy(), sf.cpu().numpy())
    ref = fid_ref64(tf.cpu().numpy(), sf.cpu().numpy())
    print(f"pipeline features: device {got!r} host {host!r} yardstick {ref['fid']!r} s {ref['scale']!r}  "
          f"|device - host|/s {abs(got - host) / ref['scale']:.3g}  |device - yardstick|/s "
          f"{abs(got - ref['fid']) / ref['scale']:.3g}")
    assert ref["scale"] > 0 and abs(got - host) <= FID_TOL * ref["scale"]
    assert abs(got - ref["fid"]) <= FID_TOL * ref["scale"]
    assert got == fid_score.calculate_fid_device(tf.cpu().numpy(), sf.cpu())            # host inputs are uploaded


def test_calculate_and_visualize_fid_on_the_device(weights, tmp_path, capsys, monkeypatch):
    cfg, teacher, (student,) = _diffusion_models()
    monkeypatch.setattr(fid_score, "calculate_fid", lambda *a: pytest.fail("the host formula was reached"))
    torch.manual_seed(31)
    res = fid_score.calculate_and_visualize_fid(teacher, student, cfg, output_dir=str(tmp_path), size_factor=0.05,
                                                weights=weights, stats="device")
    out = capsys.readouterr().out
    monkeypatch.undo()
    m = fid_score.InceptionModel(DEV, weights=weights)
    torch.manual_seed(31)
    tf, sf = _pipeline_features(teacher, cfg, 5, m), _pipeline_features(student, cfg, 5, m)
    want = fid_score.calculate_fid_device(tf, sf)
    assert set(res) == {"fid_score"} and isinstance(res["fid_score"], float) and res["fid_score"] == want
    ref = fid_ref64(tf.cpu().numpy(), sf.cpu().numpy())
    assert abs(want - ref["fid"]) <= FID_TOL * ref["scale"]
    with open(tmp_path / "fid_score_size_0.05.txt", "rb") as f:
        assert f.read() == f"FID Score: {want:.4f}\n".encode()
    for line in ("Calculating FID scores for size factor 0.05...", "  Generating samples from teacher model...",
                 "  Generating samples from student model...", "  Extracting features using InceptionV3...",
                 "  Calculating FID score...", f"  FID score for size factor 0.05: {want:.4f}"):
        assert line in out.splitlines(), line
    # the environment switch is the keyword's default
    monkeypatch.setenv("DT_FID_STATS", "device")
    torch.manual_seed(31)
    env = fid_score.calculate_and_visualize_fid(teacher, student, cfg, output_dir=str(tmp_path), size_factor=0.05,
                                                weights=weights)
    assert env["fid_score"] == want


def test_compute_fid_on_the_device(weights):
    from distillation_trajectories_amd.evaluation.metrics import compute_fid
    real = [(_images(1, 16, 16, seed=40 + i) + 1) / 2 for i in range(6)]
    gen = [(_images(1, 16, 16, seed=60 + i) + 1) / 2 for i in range(5)]
    fid = compute_fid(real, gen, DEV, batch_size=4, weights=weights, stats="device")
    m = fid_score.InceptionModel(DEV, weights=weights)
    fr, fg = fid_score.extract_features(torch.cat(real), m), fid_score.extract_features(torch.cat(gen), m)
    assert isinstance(fid, float) and fid == fid_score.calculate_fid_device(fr, fg)
    ref = fid_ref64(fr.cpu().numpy(), fg.cpu().numpy())
    host = compute_fid(real, gen, DEV, batch_size=4, weights=weights)
    print(f"compute_fid: device {fid!r} host {host!r} yardstick {ref['fid']!r} s {ref['scale']!r}")
    assert abs(fid - ref["fid"]) <= FID_TOL * ref["scale"]
    assert abs(fid - host) <= FID_TOL * ref["scale"]


def test_fid_sweep_equals_separate_calls(weights):
    cfg, teacher, students = _diffusion_models(n_students=3)
    torch.manual_seed(77)
    res = fid_score.fid_sweep(teacher, students, cfg, 5, weights=weights)
    assert res["fid"].shape == (3,) and res["parts"].shape == (3, 4) and res["status"].tolist() == [0, 0, 0]
    assert res["fid"].dtype == np.float64 and isinstance(res["fid"], np.ndarray)
    m = fid_score.InceptionModel(DEV, weights=weights)
    torch.manual_seed(77)
    tf = _pipeline_features(teacher, cfg, 5, m)
    for i, s in enumerate(students):
        sf = _pipeline_features(s, cfg, 5, m)
        one = engine.device_fid(tf, sf)
        assert fid_score.calculate_fid_device(tf, sf) == res["fid"][i], i
        assert _same_bits(one["parts"][0].cpu().numpy(), res["parts"][i]), i
        ref = fid_ref64(tf.cpu().numpy(), sf.cpu().numpy())
        assert abs(res["fid"][i] - ref["fid"]) <= FID_TOL * ref["scale"], i
    assert len(set(res["fid"].tolist())) == 3
