"""CPU: the float64 yardstick of the sample-quality scores (quality_ref64) against brute-force loops, its two distance
forms against each other, the documented recipe of the KID subset tables, the gap precondition of every GPU case of
tests/test_hip_quality.py (so a bad input shows here, without a GPU), the argument checks of ``engine.device_quality`` that
come before the device is touched, and the new header against the library and the binding."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import quality_ref64 as q
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.analysis.metrics import sample_quality
from fid_ref64 import feature_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dt_hip_quality.h")
MIN_GAP = 100.0


def _brute(a, b, k):
    """the definitions of include/dt_hip_quality.h as plain Python loops over float64 scalars"""
    a, b = [[float(v) for v in row] for row in a], [[float(v) for v in row] for row in b]
    D = len(a[0])

    def d2(x, y):
        return sum((u - v) ** 2 for u, v in zip(x, y))

    def kap(x, y):
        return (sum(u * v for u, v in zip(x, y)) / D + 1.0) ** 3

    ra = [sorted(d2(x, y) for y in a)[k] for x in a]
    rb = [sorted(d2(x, y) for y in b)[k] for x in b]
    precision = sum(any(d2(x, y) < ra[i] for i, x in enumerate(a)) for y in b)
    recall = sum(any(d2(x, y) < rb[j] for j, y in enumerate(b)) for x in a)
    density = sum(d2(x, y) < ra[i] for i, x in enumerate(a) for y in b)
    coverage = sum(min(d2(x, y) for y in b) < ra[i] for i, x in enumerate(a))
    n_a, n_b = len(a), len(b)
    saa = sum(kap(a[i], a[j]) for i in range(n_a) for j in range(n_a) if i != j)
    sbb = sum(kap(b[i], b[j]) for i in range(n_b) for j in range(n_b) if i != j)
    sab = sum(kap(x, y) for x in a for y in b)
    kid = saa / (n_a * (n_a - 1)) + sbb / (n_b * (n_b - 1)) - 2.0 * sab / (n_a * n_b)
    return ra, rb, [precision, recall, density, coverage], kid


@pytest.mark.parametrize("mode,k", [("same", 1), ("same", 3), ("shift", 3), ("collapse", 2), ("spread", 8)])
def test_yardstick_against_brute_force_loops(mode, k):
    a, b = q.feature_pair(3, 12, 9, 8, mode, 1)
    ra, rb, counts, kid = _brute(a, b, k)
    for form in ("direct", "gram"):
        r = q.quality_ref64(a, b, k, form=form)
        assert r["counts"].tolist() == counts, form
        assert np.allclose(r["radii_a"], ra, rtol=1e-12, atol=1e-15) and np.allclose(r["radii_b"], rb, rtol=1e-12, atol=1e-15)
        assert abs(r["kid"] - kid) <= r["kid_tol"], (form, r["kid"], kid)


@pytest.mark.parametrize("name", ["50x50", "8x50_P3", "7x6_kmax", "D80_65x64_P2", "D36_129x63"])
def test_the_two_distance_forms_agree(name):
    a, bs, k, refs = q.shape_case(name)
    for b, ref in zip(bs, refs):
        other = q.quality_ref64(a, b, k, form="gram")
        worst = max(np.abs(other["radii_a"] - ref["radii_a"]).max(), np.abs(other["radii_b"] - ref["radii_b"]).max())
        print(f"{name}: direct and Gram radii differ by {worst / ref['d2_bound']:.3g} bounds")
        assert worst <= ref["d2_bound"]
        assert other["counts"].tolist() == ref["counts"].tolist()
        centre = np.concatenate([a, b]).astype(np.float64).mean(axis=0)
        assert np.abs(q.d2_gram(a, b, centre) - q.d2_direct(a, b)).max() <= ref["d2_bound"]


def test_what_the_input_modes_give():
    far = q.quality_ref64(feature_like(1, 50, 2048), feature_like(2, 50, 2048), 5)
    assert far["counts"].tolist() == [0, 0, 0, 0] and 0.1 < far["kid"] < 0.2          # two pools: good for KID only
    a, b = q.feature_pair(5, 50, 50, 2048)
    same = q.quality_ref64(a, b, 5)["counts"]
    assert all(0 < c for c in same) and same[0] < 50 and same[1] < 50 and same[3] < 50, same
    a, b = q.feature_pair(5, 50, 50, 2048, "collapse", 0)
    c = q.quality_ref64(a, b, 5)["counts"]
    assert c[0] == 50 and c[1] == 0, c                                               # precision 1, recall 0
    a, b = q.feature_pair(5, 50, 50, 2048, "spread", 1)
    c = q.quality_ref64(a, b, 5)["counts"]
    assert c[0] == 0 and c[1] == 50, c


@pytest.mark.parametrize("name", list(q.SHAPES))
def test_gap_precondition_of_the_shape_cases(name):
    a, bs, k, refs = q.shape_case(name)
    for p, ref in enumerate(refs):
        print(f"{name}[{p}]: counts {ref['counts'].tolist()} comparison gap {ref['min_gap']:.3g} bounds, selection gap "
              f"{ref['selection_gap']:.3g} bounds, kid {ref['kid']:.3g} +- {ref['kid_tol']:.3g}")
        assert ref["ties"] == 0 and ref["min_gap"] >= MIN_GAP, (name, p, ref["min_gap"])


@pytest.mark.parametrize("name", list(q.SPECIAL))
def test_gap_precondition_of_the_degenerate_cases(name):
    a, b, k, ref = q.special_case(name)
    print(f"{name}: counts {ref['counts'].tolist()} comparison gap {ref['min_gap']:.3g} bounds, {ref['ties']} exact ties")
    assert ref["min_gap"] >= MIN_GAP
    if name == "identical":
        n = len(a)
        assert ref["counts"].tolist() == [n, n, n * k, n] and ref["ties"] == 2 * n     # each k-th neighbour, on the radius
    if name.startswith("constant"):
        assert (ref["radii_a" if name == "constant_a" else "radii_b"] == 0.0).all()
        assert ref["counts"].tolist() == [0, 0, 0, 0]


def test_subset_tables_follow_the_documented_recipe():
    ia, ib = sample_quality.kid_subset_tables(50, 70, 7, 20, seed=3)
    assert ia.shape == ib.shape == (7, 20) and ia.dtype == ib.dtype == np.int32
    rs = np.random.RandomState(3)
    for s in range(7):
        assert np.array_equal(ia[s], rs.permutation(50)[:20]) and np.array_equal(ib[s], rs.permutation(70)[:20])
        assert len(set(ia[s])) == len(set(ib[s])) == 20
    again = sample_quality.kid_subset_tables(50, 70, 7, 20, seed=3)
    assert np.array_equal(again[0], ia) and np.array_equal(again[1], ib)
    assert not np.array_equal(sample_quality.kid_subset_tables(50, 70, 7, 20, seed=4)[0], ia)
    with pytest.raises(ValueError, match="subset_size"):
        sample_quality.kid_subset_tables(50, 70, 7, 51)
    with pytest.raises(ValueError, match="num_subsets"):
        sample_quality.kid_subset_tables(50, 70, 0, 20)


def test_device_quality_names_the_offending_argument():
    a, b = torch.zeros(10, 8), torch.zeros(12, 8)
    ia, ib = sample_quality.kid_subset_tables(10, 12, 3, 5)
    for args, kw, match in (((a.double(), b), {}, "a must be float32"), ((a, b[:, :4]), {}, "feature width"),
                            ((a, torch.zeros(1, 8)), {}, "b holds 1 rows"), ((a, torch.zeros(2049, 8)), {}, "b holds 2049"),
                            ((a, b), {"k": 10}, "k=10"), ((a, b), {"k": 0}, "k=0"), ((a, b), {"k": 2.0}, "k=2.0"),
                            ((torch.zeros(2, 10, 8), torch.zeros(3, 12, 8)), {}, "number of problems"),
                            ((a, torch.zeros(12, 6)), {}, "feature width"),
                            ((a, b), {"subsets": (ia,)}, "pair"), ((a, b), {"subsets": (ia, ib[:2])}, "does not match"),
                            ((a, b), {"subsets": (ia.astype(np.float32), ib)}, r"subsets\[0\]"),
                            ((a, b), {"subsets": (ia, np.zeros((3, 11), np.int32) + np.arange(11))}, "does not match"),
                            ((a, b), {"events": [None] * 3}, "events")):
        with pytest.raises(ValueError, match=match):
            engine.device_quality(*args, **kw)
    rep, out = ia.copy(), ib.copy()
    rep[1, 4] = rep[1, 0]
    out[2, 2] = 12
    with pytest.raises(ValueError, match=r"subsets\[0\] repeats"):
        engine.device_quality(a, b, subsets=(rep, ib))
    with pytest.raises(ValueError, match=r"subsets\[1\] holds an index outside"):
        engine.device_quality(a, b, subsets=(torch.from_numpy(ia), torch.from_numpy(out)))
    with pytest.raises(engine.HipLibraryError):                                      # host tensors: no CPU fallback
        engine.device_quality(a, b, subsets=(ia, ib))


# ---------------------------------------------------------------------- header, library, binding
def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib_path():
    from distillation_trajectories_amd.csrc.build import LIB, build
    return build() if not os.path.exists(LIB) else LIB


def test_library_exports_and_binding_lists_what_the_header_declares(lib_path):
    names = declared_functions()
    assert names == ["dt_quality_scores", "dt_quality_workspace_bytes"]
    assert sorted(_hip.QUALITY_SIGNATURES) == names
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    lib = _hip.load(lib_path)
    assert lib.dt_abi_version() == _hip.ABI_VERSION == 6
    text = open(HEADER).read()
    for macro, value in (("DT_QUALITY_MAX_ROWS", engine.QUALITY_MAX_ROWS), ("DT_QUALITY_EVENTS", engine.QUALITY_EVENTS),
                         ("DT_QUALITY_MAX_SUBSETS", engine.QUALITY_MAX_SUBSETS)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value


def test_workspace_query_knows_the_limits(lib_path):
    ws = _hip.load(lib_path).dt_quality_workspace_bytes
    assert ws(1, 2, 2, 4) > 0 and ws(65535, 2, 2, 4) > 0 and ws(1, 2048, 2048, 1 << 20) > 3 * 2048 * 2048 * 8
    for bad in ((0, 50, 50, 2048), (65536, 50, 50, 2048), (1, 1, 50, 2048), (1, 50, 2049, 2048), (1, 50, 50, 2046),
                (1, 50, 50, 0), (1, 50, 50, (1 << 20) + 4)):
        assert ws(*bad) == 0, bad
    assert ws(3, 50, 60, 64) - ws(2, 50, 60, 64) >= (50 * 50 + 60 * 60 + 50 * 60) * 8    # each problem its own matrices


def test_quality_kernels_neither_spill_nor_use_scratch():
    from distillation_trajectories_amd.csrc import build
    try:
        build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.kernel_resources("dt_quality.hip")
    mine = {name: r for name, r in res.items() if name.startswith("quality_")}
    assert len(mine) == 7, sorted(res)
    for name, r in mine.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes"] == 0, (name, r)
        assert r["lds_bytes"] <= 64 * 1024, (name, r)
