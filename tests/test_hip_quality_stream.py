"""GPU: the row-panel route of the device sample-quality scores (include/dt_hip_quality_stream.h,
csrc/dt_quality_stream.hip, engine.device_quality_stream / device_quality_auto and the drivers of
analysis/metrics/sample_quality.py) against the float64 yardstick quality_ref64 on the cases of quality_stream_cases: sets
longer than the old route's 2048 rows, the exact integer ramp, identical and duplicated sets, bit-identity across
panel_rows, workspace contents, sharing, batching, strides and calls, agreement with the old route where both apply, the
status words, the stage events, the subset KIDs of the auto entry and the drivers.

Bounds (quality_ref64's docstring derives them; u = 2^-53): a squared radius within 4 (D + 4) u max |row|^2 of its set, KID
within 4 (3 (D + 2) + n_a + n_b) u S_kappa; counts exactly, after the yardstick alone has shown that every comparison that
is not an exact tie is decided by at least 100 bounds.  The dot-product bound behind the first two holds for any order of
summation, so it covers the matrix instruction's order as it covers the old route's FMA chain.  Every case prints its
deviations, in units of its bound, before it asserts."""
import numpy as np
import pytest
import torch

import quality_ref64 as q
import quality_stream_cases as cases
from distillation_trajectories_amd import engine
from distillation_trajectories_amd.analysis.metrics import sample_quality

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
MIN_GAP = 100.0
FIELDS = ("kid", "kid_subsets", "counts", "precision", "recall", "density", "coverage", "status", "radii_a", "radii_b")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _same(r1, r2, fields=FIELDS, rows=slice(None)):
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


@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_cases_match_ref64_both_ways_round(name):
    n_a, n_b, P, D, k = cases.SHAPES[name]
    a, bs, k, refs = cases.shape_case(name)
    ta = _dev(a)                                                              # 2-D: shared by all P problems
    tb = _dev(np.stack(bs)) if P > 1 else _dev(bs[0])
    r = engine.device_quality_stream(ta, tb, k=k, radii=True)                 # the default panel_rows
    assert r["kid"].shape == (P,) and r["kid_subsets"].shape == (P, 0) and r["counts"].shape == (P, 4)
    assert r["radii_a"].shape == (P, n_a) and r["radii_b"].shape == (P, n_b) and r["status"].shape == (P,)
    assert r["kid"].dtype == torch.float64 and r["counts"].dtype == torch.int64 and r["precision"].dtype == torch.float64
    for p in range(P):
        _check(r, p, a, bs[p], k, refs[p], (name, p))
    assert "radii_a" not in engine.device_quality_stream(ta, tb, k=k)
    auto = engine.device_quality_auto(ta, tb, k=k, radii=True)
    if engine.quality_route(n_a, n_b, k) == "panels":
        assert _same(auto, r)
    r2 = engine.device_quality_stream(tb, ta, k=k, radii=True)                # the sets the other way round
    for p in range(P):
        c, c2 = r["counts"][p].tolist(), r2["counts"][p].tolist()
        dk = abs(float(r2["kid"][p]) - refs[p]["kid"]) / refs[p]["kid_tol"]
        print(f"{name}[{p}] swapped: counts {c2}, kid off by {dk:.3g} bounds")
        assert (c2[0], c2[1]) == (c[1], c[0]), (name, p, c, c2)                # precision and recall swap
        assert dk <= 1.0, (name, p, dk)
        assert torch.equal(r2["radii_a"][p], r["radii_b"][p]) and torch.equal(r2["radii_b"][p], r["radii_a"][p])


@pytest.mark.parametrize("n_a,n_b", cases.RAMPS)
def test_ramp_is_exact(n_a, n_b):
    a, b, k, ref = cases.ramp(n_a, n_b)
    for rows in (None, 64):
        r = engine.device_quality_stream(_dev(a), _dev(b), k=k, radii=True, panel_rows=rows)
        ra, rb = r["radii_a"][0].cpu().numpy(), r["radii_b"][0].cpu().numpy()
        print(f"ramp {n_a}x{n_b} panel_rows={rows}: counts {r['counts'][0].tolist()} ref {ref['counts'].tolist()}, radii differ "
              f"in {int((ra != ref['radii_a']).sum())} + {int((rb != ref['radii_b']).sum())} places, row 0 / last of A "
              f"{ra[0]} / {ra[-1]}")
        assert int(r["status"][0]) == 0
        assert np.array_equal(ra, ref["radii_a"]) and np.array_equal(rb, ref["radii_b"])
        assert ra[0] == ra[-1] == 125.0 and ra[1] == 80.0 and ra[n_a // 2] == 45.0
        assert r["counts"][0].tolist() == ref["counts"].tolist() == cases.RAMP_COUNTS[(n_a, n_b)]


def test_identical_and_duplicated_sets():
    a, b, k, ref = q.special_case("identical")
    n = len(a)
    r = engine.device_quality_stream(_dev(a), _dev(b), k=k, radii=True)
    _check(r, 0, a, b, k, ref, "identical")
    assert r["counts"][0].tolist() == [n, n, n * k, n]
    assert [float(r[f][0]) for f in ("precision", "recall", "density", "coverage")] == [1.0, 1.0, 1.0, 1.0]
    assert torch.equal(r["radii_a"], r["radii_b"])
    for name in ("copies", "x4", "constant_a", "constant_b"):
        a, b, k, ref = q.special_case(name)
        r = engine.device_quality_stream(_dev(a), _dev(b), k=k, radii=True)
        _check(r, 0, a, b, k, ref, name)
        if name.startswith("constant"):                     # radii 0, nothing is < 0, no error
            assert (r["radii_a" if name == "constant_a" else "radii_b"] == 0.0).all()
            assert r["counts"][0].tolist() == [0, 0, 0, 0]


def test_bits_do_not_depend_on_panel_rows_workspace_sharing_batch_strides_or_calls():
    n_a, n_b, D, P, k = 2200, 1900, 64, 3, 5           # A needs a refill of the selection's buffer, B does not
    a = _dev(q.feature_pair(21, n_a, n_b, D)[0])
    bs = _dev(np.stack([q.feature_pair(21, n_a, n_b, D, q.MODES[p % 4], p // 4)[1] for p in range(P)]))
    kw = dict(k=k, radii=True)
    big = engine.device_quality_stream(a, bs, **kw)                            # teacher shared, the default panel
    assert len({tuple(c) for c in big["counts"].tolist()}) == P
    for rows in (64, 128, 1024, 4096):
        assert _same(engine.device_quality_stream(a, bs, panel_rows=rows, **kw), big), rows
    again = engine.device_quality_stream(a, bs, **kw)
    copied = engine.device_quality_stream(a.unsqueeze(0).repeat(P, 1, 1), bs, **kw)       # teacher copied P times
    expanded = engine.device_quality_stream(a.unsqueeze(0).expand(P, n_a, D), bs, **kw)   # a stride-0 view
    assert _same(again, big) and _same(copied, big) and _same(expanded, big)
    for p in range(P):
        assert _same(engine.device_quality_stream(a, bs[p], **kw), big, rows=slice(p, p + 1)), p
    assert _same(engine.device_quality_stream(a, bs[::2], panel_rows=128, **kw), big, rows=slice(None, None, 2))
    # rows of a wider tensor
    wide_a = torch.zeros(n_a, D + 8, device=DEV)
    wide_a[:, :D] = a
    wide_b = torch.full((P, n_b + 3, D + 8), float("nan"), device=DEV)
    wide_b[:, 1:n_b + 1, 4:D + 4] = bs
    va, vb = wide_a[:, :D], wide_b[:, 1:n_b + 1, 4:D + 4]
    assert not va.is_contiguous() and not vb.is_contiguous()
    assert _same(engine.device_quality_stream(va, vb, **kw), big)
    # a poisoned workspace, an exactly-sized one, and a short one
    nbytes = engine._hip.load().dt_quality_stream_workspace_bytes(P, n_a, n_b, D, 128)
    ws = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    assert _same(engine.device_quality_stream(a, bs, panel_rows=128, workspace=ws, **kw), big)
    exact = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    assert _same(engine.device_quality_stream(a, bs, panel_rows=128, workspace=exact, **kw), big)
    with pytest.raises(ValueError, match="workspace"):
        engine.device_quality_stream(a, bs, panel_rows=128, workspace=ws[:nbytes - 8], **kw)
    assert _same(engine.device_quality_stream(a, bs, **kw), big)


@pytest.fixture(scope="module")
def square_2048():
    """(a, b, k, yardstick) of 2048 x 2048 at D = 64: the largest shape both routes take"""
    a, b = q.feature_pair(7000 + 13 * 2048 + 2048 + 64, 2048, 2048, 64)
    return a, b, 5, q.quality_ref64(a, b, 5)


@pytest.mark.parametrize("name", ["130x70_D2048", "2048x2048_D64"])
def test_agrees_with_the_old_route_where_both_apply(name, square_2048):
    if name == "2048x2048_D64":
        a, b, k, ref = square_2048
    else:
        a, bs, k, refs = cases.shape_case(name)
        b, ref = bs[0], refs[0]
    assert ref["min_gap"] >= MIN_GAP, ref["min_gap"]
    ta, tb = _dev(a), _dev(b)
    old = engine.device_quality(ta, tb, k=k, radii=True)
    new = engine.device_quality_stream(ta, tb, k=k, radii=True)
    assert _same(engine.device_quality_auto(ta, tb, k=k, radii=True), old)     # a shape the old route took keeps its bits
    ba, bb = q.radius_bounds(a, b)
    da = float((new["radii_a"] - old["radii_a"]).abs().max()) / ba
    db = float((new["radii_b"] - old["radii_b"]).abs().max()) / bb
    dk = abs(float(new["kid"][0]) - float(old["kid"][0])) / ref["kid_tol"]
    print(f"{name}: the two routes differ by {da:.3g} / {db:.3g} bounds in the radii, {dk:.3g} bounds in KID; counts "
          f"{new['counts'][0].tolist()} (comparison gap {ref['min_gap']:.3g} bounds)")
    assert new["counts"][0].tolist() == old["counts"][0].tolist() == ref["counts"].tolist()
    assert da <= 2.0 and db <= 2.0 and dk <= 2.0                               # the sum of the two routes' bounds
    _check(new, 0, a, b, k, ref, name)


def test_status_words_isolate_bad_problems():
    n_a, n_b, D, P, k = 300, 200, 64, 5, 3
    a = q.feature_pair(12, n_a, n_b, D)[0]
    bs = np.stack([q.feature_pair(12, n_a, n_b, D, "shift", p)[1] for p in range(P)])
    ta, tb = _dev(a), _dev(bs)
    kw = dict(k=k, radii=True, panel_rows=128)
    clean = engine.device_quality_stream(ta, tb, **kw)
    assert clean["status"].cpu().tolist() == [0] * P

    def check(r, bad):
        assert r["status"].cpu().tolist() == [int(p in bad) for p in range(P)]
        for p in range(P):
            if p in bad:
                for f in ("kid", "precision", "recall", "density", "coverage"):
                    assert torch.isnan(r[f][p]), (p, f)
                for f in ("radii_a", "radii_b"):
                    assert torch.isnan(r[f][p]).all(), (p, f)
                assert r["counts"][p].tolist() == [-1] * 4
            else:
                one = {f: v[p:p + 1] for f, v in r.items()}
                assert _same(one, clean, rows=slice(p, p + 1)), p

    bad = tb.clone()
    bad[1, 7, 60] = float("nan")                                   # a NaN in one student: its neighbours keep their bits
    bad[3, n_b - 1, 63] = float("-inf")
    check(engine.device_quality_stream(ta, bad, **kw), (1, 3))
    ab = ta.unsqueeze(0).repeat(P, 1, 1)                           # a NaN in the copy of A of one problem only
    ab[2, n_a - 1, 1] = float("nan")
    check(engine.device_quality_stream(ab, tb, **kw), (2,))
    shared = ta.clone()                                            # an Inf in the shared teacher: every problem is bad
    shared[129, 5] = float("inf")
    check(engine.device_quality_stream(shared, tb, **kw), tuple(range(P)))
    check(engine.device_quality_stream(ta, tb, **kw), ())


def test_events_bracket_the_stages():
    a, b = (_dev(x) for x in q.feature_pair(41, 300, 200, 64))
    plain = engine.device_quality_stream(a, b, radii=True)
    n = engine.QUALITY_STREAM_EVENTS
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
    timed = engine.device_quality_stream(a, b, radii=True, events=ev)
    torch.cuda.synchronize()
    assert n == 6 and all(ev[i].elapsed_time(ev[i + 1]) >= 0.0 for i in range(n - 1))
    assert ev[0].elapsed_time(ev[-1]) > 0.0
    assert _same(plain, timed)
    with pytest.raises(ValueError, match="events"):
        engine.device_quality_stream(a, b, events=ev[:5])


@pytest.fixture(scope="module")
def feature_sets_2100():
    """(a, b, k, yardstick): two feature-like sets of 2100 rows, D = 64, the second shifted"""
    a, b = q.feature_pair(77, 2100, 2100, 64, "shift", 0)
    return a, b, 5, q.quality_ref64(a, b, 5)


def test_auto_serves_subsets_on_the_panel_route(feature_sets_2100):
    a, b, k, ref = feature_sets_2100
    S, m, D = 5, 50, a.shape[1]
    ia, ib = sample_quality.kid_subset_tables(len(a), len(b), S, m, seed=9)
    ta, tb = _dev(a), _dev(b)
    r = engine.device_quality_auto(ta, tb, k=k, subsets=(ia, ib), radii=True)
    assert r["kid_subsets"].shape == (1, S)
    assert _same(engine.device_quality_stream(ta, tb, k=k, radii=True), r, tuple(f for f in FIELDS if f != "kid_subsets"))
    for s in range(S):
        want, s_kappa = q.kid_ref64(a[ia[s]], b[ib[s]])
        tol = q.kid_tolerance(m, m, D, s_kappa)
        got = float(r["kid_subsets"][0, s])
        print(f"subset {s}: {got!r} ref {want!r} off by {abs(got - want) / tol:.3g} bounds")
        assert abs(got - want) <= tol, s
    with pytest.raises(ValueError, match="2048"):
        engine.device_quality_auto(ta, tb, subsets=sample_quality.kid_subset_tables(len(a), len(b), 2, 2100))


def test_drivers_give_the_yardsticks_numbers_on_2100_rows(feature_sets_2100):
    a, b, k, ref = feature_sets_2100
    n = float(len(a))
    assert ref["min_gap"] >= MIN_GAP, ref["min_gap"]
    prdc = sample_quality.calculate_prdc_device(a, b, k=k)
    kid = sample_quality.calculate_kid_device(_dev(a), _dev(b))
    c = ref["counts"].astype(np.float64)
    print(f"2100 x 2100: prdc {prdc} ref counts {ref['counts'].tolist()} (comparison gap {ref['min_gap']:.3g} bounds); kid "
          f"{kid['kid']!r} ref {ref['kid']!r} off by {abs(kid['kid'] - ref['kid']) / ref['kid_tol']:.3g} bounds")
    assert prdc == {"precision": c[0] / n, "recall": c[1] / n, "density": c[2] / (k * n), "coverage": c[3] / n}
    assert abs(kid["kid"] - ref["kid"]) <= ref["kid_tol"] and np.isnan(kid["kid_mean"]) and np.isnan(kid["kid_std"])
    sub = sample_quality.calculate_kid_device(a, b, num_subsets=3, subset_size=40, seed=2)
    ia, ib = sample_quality.kid_subset_tables(len(a), len(b), 3, 40, seed=2)
    want = [q.kid_ref64(a[ia[s]], b[ib[s]]) for s in range(3)]
    tol = max(q.kid_tolerance(40, 40, a.shape[1], s_kappa) for _, s_kappa in want)
    assert sub["kid"] == kid["kid"]
    assert abs(sub["kid_mean"] - np.mean([w for w, _ in want])) <= tol and abs(sub["kid_std"] - np.std([w for w, _ in want])) <= tol
