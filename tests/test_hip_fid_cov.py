"""GPU: the feature-space route of the device Fréchet distance (include/dt_hip_fid_cov.h, csrc/dt_fid.hip,
engine.device_fid_cov) against the float64 yardstick fid_ref64: the listed shapes (sets shorter than the width, whose
covariances drop pivots, among them), agreement with the sample-space route where both apply, degenerate inputs, the status
word, bit-identity across batching, sharing, strides, calls and workspace contents, and the driver on sets the sample-space
route refuses.

Bounds (s = tr S_a + tr S_b from the yardstick).  Full-rank cases and the listed shapes: fid and the cross term within
1e-6 s, the standing bound of tests/test_hip_fid.py; |mu_a - mu_b|^2 and the traces within 1e-9 relative.  The two routes
against each other: 2e-6 s.  Degenerate inputs: 1e-6 s + 2 z 2^-26 sigma_max / sqrt((n_a - 1)(n_b - 1)), with sigma_max the
largest singular value of the yardstick's A_c B_c^T and z = D - (the number of its singular values above 1e-12 sigma_max):
bisection returns each exactly-zero eigenvalue of the squared matrix as +- a few eps lambda_max, whose square root is up
to sqrt(eps) sigma_max; the margin is twice that mechanism.  Every case prints its deviation before it asserts."""
import functools

import numpy as np
import pytest
import torch

from distillation_trajectories_amd import engine
from distillation_trajectories_amd.analysis.metrics import fid_score
from fid_ref64 import feature_like, fid_ref64

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
FID_TOL = 1e-6
PART_TOL = 1e-9
ROUTES_TOL = 2e-6

SHAPES = {
    "D4_5x7": dict(n_a=5, n_b=7, P=1, D=4),
    "D64_300x257_P2": dict(n_a=300, n_b=257, P=2, D=64),
    "D36_129x63": dict(n_a=129, n_b=63, P=1, D=36),
    "D80_65x64_P2": dict(n_a=65, n_b=64, P=2, D=80),             # n < D: dropped pivots, a second panel of 16 columns
    "D80_64x65_P2": dict(n_a=64, n_b=65, P=2, D=80),
    "D68_200x130_P3": dict(n_a=200, n_b=130, P=3, D=68),         # one quad into the second panel
    "D132_200x130_P3": dict(n_a=200, n_b=130, P=3, D=132),       # three panels, a trailing update past the first
    "D64_2500x2300": dict(n_a=2500, n_b=2300, P=1, D=64),        # what the sample-space route refuses; five row slabs
    "D2048_2100x2100": dict(n_a=2100, n_b=2100, P=1, D=2048),    # full width
}
BOTH_ROUTES = list(SHAPES)[:-2]


@functools.lru_cache(maxsize=None)
def _case(name):
    """the host rows of a shape and the yardstick of each of its problems, computed once"""
    sh = SHAPES[name]
    n_a, n_b, P, D = sh["n_a"], sh["n_b"], sh["P"], sh["D"]
    a = feature_like(1000 + n_a, n_a, D)
    bs = [feature_like(2000 + n_b + p, n_b, D, shift=0.01 * (p + 1), spread=0.15 + 0.02 * p) for p in range(P)]
    refs = [fid_ref64(a, b) for b in bs]
    for r in refs:
        r["parts"].setflags(write=False)
    return a, bs, refs


def _five(r, p=0):
    """the five doubles of problem p as one host array (fid, then the four parts)"""
    return np.concatenate([r["fid"][p:p + 1].cpu().numpy(), r["parts"][p].cpu().numpy()])


def _same_bits(x, y):
    return x.tobytes() == y.tobytes()


def _check(five, ref, what, swapped=False, extra=0.0):
    """five doubles of the device against a yardstick (of the sets the other way round if ``swapped``)"""
    s = ref["scale"]
    parts = ref["parts"][[0, 2, 1, 3]] if swapped else ref["parts"]
    dev_fid, dev_cross = abs(five[0] - ref["fid"]) / s, abs(five[4] - parts[3]) / s
    rel = [abs(five[1 + i] - parts[i]) / max(abs(parts[i]), 1e-300) for i in range(3)]
    print(f"{what}: fid {five[0]!r} ref {ref['fid']!r}  |d fid|/s {dev_fid:.3g}  |d cross|/s {dev_cross:.3g}  "
          f"parts rel {max(rel):.3g}  bound/s {FID_TOL + extra / s:.3g}")
    assert np.all(np.isfinite(five)), what
    assert dev_fid <= FID_TOL + extra / s, (what, dev_fid)
    assert dev_cross <= FID_TOL + extra / s, (what, dev_cross)
    for i, name in enumerate(("dmu2", "tr_a", "tr_b")):
        assert rel[i] <= PART_TOL, (what, name, rel[i])
    assert five[0] == five[1] + five[2] + five[3] - 2.0 * five[4], what


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_match_ref64(name):
    sh = SHAPES[name]
    P = sh["P"]
    a, bs, refs = _case(name)
    ta = torch.from_numpy(a).to(DEV)                                       # 2-D: shared by all P problems
    tb = torch.from_numpy(np.stack(bs)).to(DEV) if P > 1 else torch.from_numpy(bs[0]).to(DEV)
    r = engine.device_fid_cov(ta, tb)
    assert r["fid"].shape == (P,) and r["parts"].shape == (P, 4) and r["status"].shape == (P,)
    assert r["fid"].dtype == torch.float64 and r["parts"].dtype == torch.float64 and r["status"].dtype == torch.int32
    assert r["status"].cpu().tolist() == [0] * P
    for p in range(P):
        _check(_five(r, p), refs[p], (name, p))
    if P > 1:                                      # the sets the other way round: fid is symmetric, the traces swap
        r2 = engine.device_fid_cov(tb, ta)
        assert r2["status"].cpu().tolist() == [0] * P
        for p in range(P):
            _check(_five(r2, p), refs[p], (name, p, "swapped"), swapped=True)


@pytest.mark.parametrize("name", BOTH_ROUTES)
def test_the_two_routes_agree_where_both_apply(name):
    a, bs, refs = _case(name)
    ta = torch.from_numpy(a).to(DEV)
    for p, b in enumerate(bs):
        tb = torch.from_numpy(b).to(DEV)
        cov, old = _five(engine.device_fid_cov(ta, tb)), _five(engine.device_fid(ta, tb))
        dev = abs(cov[0] - old[0]) / refs[p]["scale"]
        print(f"{name}[{p}]: feature-space {cov[0]!r} sample-space {old[0]!r}  |difference|/s {dev:.3g}")
        assert dev <= ROUTES_TOL, (name, p, dev)


def _degenerate_extra(a, b, D):
    """(the second term of the degenerate bound, z, sigma_max), all from the yardstick's centred cross product"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    sv = np.linalg.svd((a - a.mean(axis=0)) @ (b - b.mean(axis=0)).T, compute_uv=False)
    smax = float(sv[0])
    z = D - int(np.sum(sv > 1e-12 * smax)) if smax > 0 else D
    return 2.0 * z * 2.0 ** -26 * smax / np.sqrt((len(a) - 1.0) * (len(b) - 1.0)), z, smax


def _degenerate(a, b, what):
    D = a.shape[1]
    extra, z, smax = _degenerate_extra(a, b, D)
    ref = fid_ref64(a, b)
    r = engine.device_fid_cov(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    assert r["status"].cpu().tolist() == [0]
    five = _five(r)
    print(f"{what}: z {z}  sigma_max {smax:.6g}  second term / s {extra / ref['scale']:.3g}")
    _check(five, ref, what, extra=extra)
    return five, ref


def test_degenerate_inputs():
    D = 256
    a = feature_like(5, 600, D)
    # both sets identical: 0 within rounding, possibly negative, not clamped
    five, ref = _degenerate(a, a.copy(), "identical")
    assert abs(five[0]) <= FID_TOL * ref["scale"] and five[1] == 0.0 and five[2] == five[3]
    # features in a 20-dimensional subspace: 236 pivots of each covariance drop
    lo_a, lo_b = feature_like(6, 300, D, rank=20), feature_like(7, 257, D, rank=20, shift=0.01)
    _degenerate(lo_a, lo_b, "rank 20, two subspaces")
    _degenerate(lo_a, feature_like(6, 300, D, rank=20)[:257] * np.float32(1.0), "rank 20, one subspace")
    # every row four times
    _degenerate(np.repeat(feature_like(5, 100, D), 4, axis=0), np.repeat(feature_like(8, 90, D, shift=0.02), 4, axis=0),
                "duplicated x4")


def test_sets_without_variance():
    D = 256
    a = feature_like(5, 300, D)
    const = np.full((40, D), 0.37, np.float32)
    # one constant set: no error, its trace and the cross term are exactly 0
    for x, y, tr in ((const, a, 2), (a, const, 3)):
        r = engine.device_fid_cov(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
        five = _five(r)
        _check(five, fid_ref64(x, y), "constant set")
        assert r["status"].cpu().tolist() == [0] and five[tr] == 0.0 and five[4] == 0.0
    r = engine.device_fid_cov(torch.full((40, D), 0.25, device=DEV), torch.full((9, D), 0.75, device=DEV))
    assert r["status"].cpu().tolist() == [0]
    assert np.array_equal(_five(r), [0.25 * D, 0.25 * D, 0.0, 0.0, 0.0])


def test_status_words_isolate_bad_problems():
    D, P = 256, 5
    a = feature_like(11, 30, D)
    bs = np.stack([feature_like(12 + p, 24, D, shift=0.01) for p in range(P)])
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(bs).to(DEV)
    clean = engine.device_fid_cov(ta, tb)
    assert clean["status"].cpu().tolist() == [0] * P
    bad = tb.clone()
    bad[1, 7, 100] = float("nan")
    bad[2, 23, 255] = float("inf")
    bad[4, 0, 0] = float("-inf")
    r = engine.device_fid_cov(ta, bad)
    assert r["status"].cpu().tolist() == [0, 1, 1, 0, 1]
    for p in (1, 2, 4):
        assert np.all(np.isnan(_five(r, p))), p
    for p in (0, 3):
        assert _same_bits(_five(r, p), _five(clean, p)), p
    # a NaN in set a of one problem only
    ab = ta.unsqueeze(0).repeat(P, 1, 1)
    ab[3, 29, 1] = float("nan")
    r = engine.device_fid_cov(ab, tb)
    assert r["status"].cpu().tolist() == [0, 0, 0, 1, 0]
    assert np.all(np.isnan(_five(r, 3)))
    for p in (0, 1, 2, 4):
        assert _same_bits(_five(r, p), _five(clean, p)), p


@pytest.mark.parametrize("n_a,n_b,D", [(600, 70, 132), (1100, 1030, 64)], ids=["D132_600x70", "D64_1100x1030"])
def test_bits_do_not_depend_on_batch_sharing_strides_calls_or_workspace(n_a, n_b, D):
    """D = 132: three panels, set a in two row slabs and set b in one; D = 64: three slabs each and two chunks of rows"""
    P = 5
    a = torch.from_numpy(feature_like(21, n_a, D)).to(DEV)
    bs = torch.from_numpy(np.stack([feature_like(30 + p, n_b, D, shift=0.01 * p) for p in range(P)])).to(DEV)
    big = engine.device_fid_cov(a, bs)                                             # teacher shared
    assert big["status"].cpu().tolist() == [0] * P
    again = engine.device_fid_cov(a, bs)
    copied = engine.device_fid_cov(a.unsqueeze(0).repeat(P, 1, 1), bs)             # teacher stacked P times
    expanded = engine.device_fid_cov(a.unsqueeze(0).expand(P, n_a, D), bs)         # a stride-0 view
    for f in ("fid", "parts", "status"):
        assert torch.equal(big[f], again[f]) and torch.equal(big[f], copied[f]) and torch.equal(big[f], expanded[f]), f
    for p in (0, 2, 4):
        alone = engine.device_fid_cov(a, bs[p])
        assert _same_bits(_five(alone), _five(big, p)), p
    # non-contiguous views: rows of a wider tensor (row stride D + 8) and every other problem of the batch
    wide_a = torch.zeros(n_a, D + 8, device=DEV)
    wide_a[:, :D] = a
    wide_b = torch.full((P, n_b + 3, D + 8), float("nan"), device=DEV)
    wide_b[:, 1:n_b + 1, 4:D + 4] = bs
    va, vb = wide_a[:, :D], wide_b[:, 1:n_b + 1, 4:D + 4]
    assert not va.is_contiguous() and not vb.is_contiguous()
    view = engine.device_fid_cov(va, vb)
    for f in ("fid", "parts", "status"):
        assert torch.equal(view[f], big[f]), f
    half = engine.device_fid_cov(a, bs[::2])
    assert torch.equal(half["fid"], big["fid"][::2]) and torch.equal(half["parts"], big["parts"][::2])
    # a workspace of 0xFF bytes against one of zeros
    nbytes = engine._hip.load().dt_fid_cov_workspace_bytes(P, n_a, n_b, D)
    for fill in (0xFF, 0x00):
        ws = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device=DEV)
        filled = engine.device_fid_cov(a, bs, workspace=ws)
        for f in ("fid", "parts", "status"):
            assert torch.equal(filled[f], big[f]), (f, fill)
    with pytest.raises(ValueError, match="workspace"):
        engine.device_fid_cov(a, bs, workspace=ws[:nbytes - 8])


def test_events_bracket_the_stages():
    a = torch.from_numpy(feature_like(41, 300, 64)).to(DEV)
    b = torch.from_numpy(feature_like(42, 257, 64)).to(DEV)
    plain = engine.device_fid_cov(a, b)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(engine.FID_COV_EVENTS)]
    timed = engine.device_fid_cov(a, b, events=ev)
    torch.cuda.synchronize()
    assert all(ev[i].elapsed_time(ev[i + 1]) >= 0.0 for i in range(engine.FID_COV_EVENTS - 1))
    assert ev[0].elapsed_time(ev[-1]) > 0.0
    assert _same_bits(_five(plain), _five(timed))


def test_calculate_fid_device_takes_sets_past_2048_rows():
    """two sets of 2100 rows at the full width: ``calculate_fid_device`` used to raise on them"""
    a = torch.from_numpy(feature_like(51, 2100, 2048)).to(DEV)
    b = torch.from_numpy(feature_like(52, 2100, 2048, shift=0.01)).to(DEV)
    assert engine.fid_route(2100, 2100, 2048) == "features"
    with pytest.raises(ValueError, match="2048.*feature-space"):
        engine.device_fid(a, b)
    got = fid_score.calculate_fid_device(a, b)
    direct = engine.device_fid_cov(a, b)
    auto = engine.device_fid_auto(a, b)
    assert isinstance(got, float) and np.isfinite(got) and direct["status"].cpu().tolist() == [0]
    assert _same_bits(np.float64(got), direct["fid"].cpu().numpy()[0])
    assert torch.equal(auto["fid"], direct["fid"]) and torch.equal(auto["parts"], direct["parts"])
