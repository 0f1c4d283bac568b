"""The row-panel route of the device sample-quality scores without a GPU (include/dt_hip_quality_stream.h,
engine.device_quality_stream, engine.quality_route, engine.device_quality_auto): the exported surface, the workspace query
on both sides of every limit and at its largest shape, argument checks that fail before any device call, the choice of
route and which entry the four drivers reach, the chunks of the subset path, the import surface through the reference's
module names, the resources of the new kernels, and the preconditions of the cases of tests/test_hip_quality_stream.py
(so a bad input shows here)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import quality_stream_cases as cases
from distillation_trajectories_amd import _hip, engine
from distillation_trajectories_amd.analysis.metrics import sample_quality

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dt_hip_quality_stream.h")
MIN_GAP = 100.0


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dt_[a-z0-9_]+)\s*\(", text)))


def _lib_path():
    from distillation_trajectories_amd.csrc.build import LIB, build
    return build() if not os.path.exists(LIB) else LIB


def test_header_binding_and_exports_agree():
    path = _lib_path()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dt_[a-z0-9_]+)", out))
    names = _declared()
    assert names == ["dt_quality_stream_scores", "dt_quality_stream_workspace_bytes"]
    assert sorted(_hip.QUALITY_STREAM_SIGNATURES) == names and set(names) <= exported
    assert not set(names) & set(_hip.QUALITY_SIGNATURES)
    lib = _hip.load(path)
    assert lib.dt_abi_version() == _hip.ABI_VERSION == 6
    assert all(getattr(lib, n).argtypes is not None for n in names)
    text = open(HEADER).read()
    for macro, value in (("DT_QUALITY_STREAM_MAX_ROWS", engine.QUALITY_STREAM_MAX_ROWS),
                         ("DT_QUALITY_STREAM_MAX_K", engine.QUALITY_STREAM_MAX_K),
                         ("DT_QUALITY_STREAM_EVENTS", engine.QUALITY_STREAM_EVENTS)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value
    assert (engine.QUALITY_STREAM_MAX_ROWS, engine.QUALITY_STREAM_MAX_K, engine.QUALITY_STREAM_EVENTS) == (131072, 1023, 6)
    from distillation_trajectories_amd.csrc import build
    assert any(h.endswith("dt_hip_quality_stream.h") for h in build.HEADERS) and "dt_quality_stream.hip" in build.SOURCES


def test_workspace_query_on_both_sides_of_every_limit():
    ws = _hip.load(_lib_path()).dt_quality_stream_workspace_bytes
    for ok in ((1, 2, 2, 4, 64), (65535, 2, 2, 4, 64), (1, 131072, 2, 4, 64), (1, 2, 131072, 4, 4096), (1, 50, 50, 1 << 20, 64),
               (1, 2049, 2049, 2048, 1024), (1, 50, 50, 2048, 4096)):
        assert ws(*ok) > 0, ok
    for bad in ((0, 50, 50, 2048, 64), (65536, 50, 50, 2048, 64), (1, 1, 50, 2048, 64), (1, 50, 1, 2048, 64),
                (1, 131073, 50, 2048, 64), (1, 50, 131073, 2048, 64), (1, 50, 50, 2046, 64), (1, 50, 50, 0, 64),
                (1, 50, 50, (1 << 20) + 4, 64), (1, 50, 50, 2048, 0), (1, 50, 50, 2048, 63), (1, 50, 50, 2048, 96),
                (1, 50, 50, 2048, 4160), (1, 50, 50, 2048, -64), (1, -5, 50, 2048, 64)):
        assert ws(*bad) == 0, bad


def test_workspace_grows_by_the_panel_and_never_by_n_squared():
    ws = _hip.load(_lib_path()).dt_quality_stream_workspace_bytes
    got = ws(65535, 131072, 131072, 4096, 4096)                   # the largest shape: no overflow
    per = 4096 * 131072 + 6 * 2 * 131072
    assert 65535 * 4096 * 131072 * 8 < got <= 65535 * per * 8 + 2 * 65535 * 4 + 256, got
    assert got > 2 ** 47
    for n_a, n_b, rows in ((50000, 10000, 1024), (10000, 50000, 512), (2049, 2049, 64), (131072, 131072, 4096)):
        one = ws(3, n_a, n_b, 2048, rows) - ws(2, n_a, n_b, 2048, rows)              # what a problem adds
        n = max(n_a, n_b)
        assert rows * n * 8 <= one <= (rows * n + 6 * (n_a + n_b)) * 8, (n_a, n_b, rows, one)
        assert ws(1, n_a, n_b, 2048, rows) == ws(1, n_a, n_b, 64, rows)              # D is not in it
    assert ws(1, 50000, 50000, 2048, 128) - ws(1, 50000, 50000, 2048, 64) == 64 * 50000 * 8
    assert ws(1, 131072, 131072, 2048, 64) < 131072 * 131072                          # far below one byte per pair


def test_bad_arguments_raise_before_any_device_call(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_hip, "load", no_load)
    a, b = torch.zeros(10, 8), torch.zeros(12, 8)
    fn = engine.device_quality_stream
    for args, kw, match in (((a.double(), b), {}, "a must be float32"), ((a, b[:, :4]), {}, "feature width"),
                            ((a, torch.zeros(1, 8)), {}, "b holds 1 rows"), ((torch.zeros(1, 8), b), {}, "a holds 1 rows"),
                            ((a, torch.zeros(131073, 4)), {}, "feature width"),
                            ((a[:, :4], torch.zeros(131073, 4)), {}, "b holds 131073 rows.*131072"),
                            ((a, b), {"k": 10}, "k=10"), ((a, b), {"k": 0}, "k=0"), ((a, b), {"k": 2.0}, "k=2.0"),
                            ((a, b), {"k": True}, "k=True"),
                            ((torch.zeros(1100, 4), torch.zeros(1100, 4)), {"k": 1024}, "k=1024.*1023"),
                            ((torch.zeros(2, 10, 8), torch.zeros(3, 12, 8)), {}, "number of problems"),
                            ((a, torch.zeros(12, 6)), {}, "feature width"),
                            ((torch.zeros(10, 6), torch.zeros(12, 6)), {}, "multiple of 4"),
                            ((a, b), {"panel_rows": 96}, "panel_rows=96"), ((a, b), {"panel_rows": 0}, "panel_rows=0"),
                            ((a, b), {"panel_rows": 4160}, "panel_rows=4160"), ((a, b), {"panel_rows": 64.0}, "panel_rows=64.0"),
                            ((a, b), {"events": [None] * 5}, "events must be 6")):
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)
    with pytest.raises(engine.HipLibraryError, match="CUDA"):                    # well-formed, but not on the device
        fn(a, b)
    with pytest.raises(engine.HipLibraryError, match="CUDA"):                    # what device_quality refuses, this takes
        fn(torch.zeros(2049, 4), torch.zeros(2049, 4), k=1023, panel_rows=4096)
    with pytest.raises(ValueError, match="b holds 2049"):                        # ... and device_quality still refuses
        engine.device_quality(torch.zeros(10, 4), torch.zeros(2049, 4))
    # device_quality_auto: the route's message, the subset checks and the subset limit, all before the device
    auto = engine.device_quality_auto
    big = torch.zeros(2049, 4)
    with pytest.raises(ValueError, match="131072"):
        auto(torch.zeros(131073, 4), big)
    with pytest.raises(ValueError, match="k=1024.*1023"):
        auto(big, big, k=1024)
    with pytest.raises(ValueError, match="a must be float32"):
        auto(big.double(), big)
    tables = sample_quality.kid_subset_tables(2049, 2049, 2, 2049)
    with pytest.raises(ValueError, match="subsets of size 2049.*2048"):
        auto(big, big, subsets=tables)
    rep = sample_quality.kid_subset_tables(2049, 2049, 2, 20)[0].copy()
    rep[1, 4] = rep[1, 0]
    with pytest.raises(ValueError, match=r"subsets\[0\] repeats"):
        auto(big, big, subsets=(rep, rep))
    with pytest.raises(engine.HipLibraryError, match="CUDA"):
        auto(big, big)
    with pytest.raises(engine.HipLibraryError, match="CUDA"):
        auto(a, b)


def test_quality_route_on_both_sides_of_each_threshold():
    route = engine.quality_route
    assert route(2048, 2048, 5) == "matrices" and route(2, 2, 1) == "matrices" and route(2048, 2048, 2047) == "matrices"
    assert route(2049, 2048, 5) == "panels" and route(2048, 2049, 5) == "panels" and route(50, 2049, 5) == "panels"
    assert route(131072, 131072, 1023) == "panels" and route(131072, 2, 1) == "panels"
    with pytest.raises(ValueError, match="2048.*131072"):
        route(131073, 50, 5)
    with pytest.raises(ValueError, match="2048.*131072"):
        route(50, 131073, 5)
    with pytest.raises(ValueError, match="k=1024.*1023"):
        route(2049, 2049, 1024)
    assert route(2048, 2048, 1024) == "matrices"                  # the old route has no such limit on k


class _Recorder:
    """the engine entries replaced by recorders of (name, shapes, keywords)"""

    def __init__(self, monkeypatch):
        self.seen = []
        for name in ("device_quality", "device_quality_stream"):
            monkeypatch.setattr(engine, name, self._quality(name))
        for name in ("device_fid", "device_fid_cov"):
            monkeypatch.setattr(engine, name, self._fid(name))
        monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)      # no device to upload to here

    def _quality(self, name):
        def fn(a, b, k=5, subsets=None, radii=False, **kw):
            P = b.shape[0] if b.dim() == 3 else (a.shape[0] if a.dim() == 3 else 1)
            S = 0 if subsets is None else len(subsets[0])
            self.seen.append((name, tuple(a.shape), tuple(b.shape), k, S))
            f64 = torch.float64
            out = {"kid": torch.arange(P, dtype=f64) + 0.25, "kid_subsets": torch.zeros(P, S, dtype=f64),
                   "counts": torch.ones(P, 4, dtype=torch.int64), "status": torch.zeros(P, dtype=torch.int32)}
            for f in ("precision", "recall", "density", "coverage"):
                out[f] = torch.full((P,), 0.5, dtype=f64)
            return out
        return fn

    def _fid(self, name):
        def fn(a, b, events=None, workspace=None):
            P = b.shape[0] if b.dim() == 3 else 1
            self.seen.append((name, tuple(a.shape), tuple(b.shape)))
            return {"fid": torch.full((P,), 1.5, dtype=torch.float64), "parts": torch.zeros(P, 4, dtype=torch.float64),
                    "status": torch.zeros(P, dtype=torch.int32)}
        return fn


def test_kid_and_prdc_drivers_reach_the_entry_the_route_names(monkeypatch):
    rec = _Recorder(monkeypatch)
    small, edge, big = (np.zeros((n, 8), np.float32) for n in (50, 2048, 2049))
    assert sample_quality.calculate_prdc_device(small, edge, k=3)["precision"] == 0.5
    assert sample_quality.calculate_prdc_device(edge, big, k=3)["recall"] == 0.5
    assert sample_quality.calculate_kid_device(edge, edge)["kid"] == 0.25
    assert sample_quality.calculate_kid_device(big, small)["kid"] == 0.25
    assert sample_quality.calculate_kid_device(small, edge, num_subsets=3, subset_size=20)["kid"] == 0.25
    assert rec.seen == [("device_quality", (50, 8), (2048, 8), 3, 0), ("device_quality_stream", (2048, 8), (2049, 8), 3, 0),
                        ("device_quality", (2048, 8), (2048, 8), 1, 0), ("device_quality_stream", (2049, 8), (50, 8), 1, 0),
                        ("device_quality", (50, 8), (2048, 8), 1, 3)]


def test_subset_path_of_the_panel_route_gathers_in_chunks_of_at_most_16(monkeypatch):
    rec = _Recorder(monkeypatch)
    n_a, n_b, S, m = 2049, 2100, 37, 50
    a = torch.arange(n_a, dtype=torch.float32)[:, None].repeat(1, 8)            # row i holds i: a gather shows its rows
    b = torch.arange(n_b, dtype=torch.float32)[None, :, None].repeat(2, 1, 8) + 0.5
    tables = sample_quality.kid_subset_tables(n_a, n_b, S, m, seed=3)
    gathered = []
    inner = engine.device_quality

    def spy(ga, gb, k=5, **kw):
        gathered.append((ga[:, :, 0].clone(), gb[:, :, 0].clone()))
        return inner(ga, gb, k=k, **kw)
    monkeypatch.setattr(engine, "device_quality", spy)
    res = engine.device_quality_auto(a, b, k=4, subsets=tables)
    assert res["kid_subsets"].shape == (2, S) and res["kid"].shape == (2,)
    assert rec.seen[0] == ("device_quality_stream", (n_a, 8), (2, n_b, 8), 4, 0)
    calls = rec.seen[1:]
    assert all(c[0] == "device_quality" and c[3] == 1 and c[4] == 0 for c in calls)          # k = 1, problems of their own
    assert [c[1][0] for c in calls] == [16, 16, 16, 16, 5, 5] and all(c[1][1:] == (m, 8) == c[2][1:] for c in calls)
    for i, (ga, gb) in enumerate(gathered):                      # chunk i // 2 of the tables, problem i % 2
        s0, p = 16 * (i // 2), i % 2
        assert np.array_equal(ga.numpy(), tables[0][s0:s0 + 16].astype(np.float32))
        assert np.array_equal(gb.numpy(), tables[1][s0:s0 + 16].astype(np.float32) + 0.5)
    # each subset's value is the kid of the gathered problem it was (the recorder numbers the problems of a call)
    assert res["kid_subsets"][0].tolist() == [s % 16 + 0.25 for s in range(S)]


@pytest.mark.parametrize("num_samples,quality,fid", [(6, "device_quality", "device_fid"), (2048, "device_quality", "device_fid"),
                                                     (2049, "device_quality_stream", "device_fid_cov")])
def test_sweeps_reach_the_entries_the_routes_name(monkeypatch, num_samples, quality, fid):
    from distillation_trajectories_amd.analysis.metrics import fid_score
    rec = _Recorder(monkeypatch)
    monkeypatch.setattr(fid_score, "generate_samples",
                        lambda model, config, n, device, fixed_samples=None: torch.zeros(n, 3, 4, 4))
    monkeypatch.setattr(fid_score, "InceptionModel", lambda device, weights=None: None)
    monkeypatch.setattr(fid_score, "extract_features", lambda samples, model, **k: torch.zeros(len(samples), 8))
    model = torch.nn.Linear(2, 2)
    res = sample_quality.quality_sweep(model, [model, model], None, num_samples, k=3)
    n = num_samples
    assert rec.seen == [(fid, (n, 8), (2, n, 8)), (quality, (n, 8), (2, n, 8), 3, 0)]
    assert res["fid"].tolist() == [1.5, 1.5] and res["kid"].tolist() == [0.25, 1.25] and res["counts"].shape == (2, 4)


@pytest.mark.parametrize("num_samples,quality,fid", [(6, "device_quality", "device_fid"),
                                                     (2049, "device_quality_stream", "device_fid_cov")])
def test_guidance_sweep_reaches_the_entries_the_routes_name(monkeypatch, num_samples, quality, fid):
    from distillation_trajectories_amd import synthetic
    from distillation_trajectories_amd.analysis import trajectory_engine
    from distillation_trajectories_amd.analysis.metrics import fid_score
    from distillation_trajectories_amd.config import Config
    rec = _Recorder(monkeypatch)
    cfg = Config()
    cfg.image_size, cfg.timesteps = 4, 2
    S, T, C = num_samples, cfg.timesteps, cfg.channels
    monkeypatch.setattr(fid_score, "InceptionModel", lambda device, weights=None: None)
    monkeypatch.setattr(fid_score, "extract_features", lambda samples, model, **k: torch.zeros(len(samples), 8))
    monkeypatch.setattr(synthetic, "noise_table", lambda seed, n, shape: torch.zeros(n, *shape))
    monkeypatch.setattr(engine.UNetHandle, "for_module", staticmethod(lambda m: m))
    monkeypatch.setattr(trajectory_engine, "sample_grid",
                        lambda handle, table, first, n, steps, scales, h, w: {gs: {steps: torch.zeros(n, C * h * w)} for gs in scales})
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    model = torch.nn.Linear(2, 2)
    res = sample_quality.guidance_quality_sweep(model, [model], cfg, (1.0, 2.0), S, k=3)
    assert rec.seen == [(quality, (S, 8), (1, S, 8), 3, 0), (fid, (S, 8), (1, S, 8))] * 2
    assert res["fid"].shape == (1, 2) and res["kid"].tolist() == [[0.25, 0.25]]


def test_new_names_import_after_aliases():
    import distillation_trajectories_amd as pkg
    pkg.remove_aliases()
    try:
        pkg.install_aliases()
        from analysis.metrics import fid_score as aliased           # the reference has no sample_quality module to alias
        from distillation_trajectories_amd.analysis.metrics.sample_quality import calculate_kid_device, calculate_prdc_device
        assert calculate_kid_device is sample_quality.calculate_kid_device
        assert calculate_prdc_device is sample_quality.calculate_prdc_device
        assert sample_quality.engine is aliased.engine is engine
        for name in ("device_quality_stream", "device_quality_auto", "quality_route", "QUALITY_STREAM_MAX_ROWS",
                     "QUALITY_STREAM_MAX_K", "QUALITY_STREAM_EVENTS"):
            assert getattr(aliased.engine, name) is getattr(engine, name), name
    finally:
        pkg.remove_aliases()


def test_stream_kernels_neither_spill_nor_use_scratch():
    from distillation_trajectories_amd.csrc import build
    try:
        build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.kernel_resources("dt_quality_stream.hip")
    mine = {name: r for name, r in res.items() if name.startswith("qstream_")}
    assert sorted(mine) == ["qstream_count_cols_kernel", "qstream_count_rows_kernel", "qstream_diag_kernel",
                            "qstream_finish_kernel", "qstream_flag_kernel", "qstream_gram_kernel", "qstream_kappa_kernel",
                            "qstream_select_kernel"], sorted(res)
    assert not [n for n in res if n.startswith("quality_")]                  # the old route's count of seven stays its own
    for name, r in mine.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes"] == 0, (name, r)
        assert r["lds_bytes"] <= 64 * 1024, (name, r)
    listed = open(os.path.join(ROOT, "profiles", "kernel_resources.txt")).read()
    assert "# dt_quality_stream.hip" in listed and all(re.search(rf"^{n}\s", listed, flags=re.M) for n in mine)


@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_gap_precondition_of_the_cases(name):
    n_a, n_b, P, D, k = cases.SHAPES[name]
    a, bs, k, refs = cases.shape_case(name)
    assert a.shape == (n_a, D) and len(bs) == P and all(b.shape == (n_b, D) for b in bs)
    for p, ref in enumerate(refs):
        print(f"{name}[{p}]: counts {ref['counts'].tolist()} comparison gap {ref['min_gap']:.3g} bounds, selection gap "
              f"{ref['selection_gap']:.3g} bounds, kid {ref['kid']:.3g} +- {ref['kid_tol']:.3g}")
        assert ref["ties"] == 0 and ref["min_gap"] >= MIN_GAP, (name, p, ref["min_gap"])
    assert k <= engine.QUALITY_STREAM_MAX_K and engine.quality_route(n_a, n_b, k) == ("panels" if max(n_a, n_b) > 2048 else "matrices")


def test_the_table_holds_the_cases_it_must():
    assert {"2049x2049_D64": (2049, 2049, 1, 64, 5), "4100x2100_P4_D128": (4100, 2100, 4, 128, 3),
            "2100x4161_D36_k63": (2100, 4161, 1, 36, 63), "2111x2065_D2048": (2111, 2065, 1, 2048, 5),
            "130x70_D2048": (130, 70, 1, 2048, 5)}.items() <= cases.SHAPES.items()
    top = [v for v in cases.SHAPES.values() if v[4] == 1023]
    assert len(top) == 1 and 2049 <= top[0][0] <= 2200 and top[0][3] <= 64
    assert set(cases.SEEDS) <= set(cases.SHAPES)


@pytest.mark.parametrize("n_a,n_b", cases.RAMPS)
def test_the_ramp_is_exact_and_gives_the_stated_counts(n_a, n_b):
    a, b, k, ref = cases.ramp(n_a, n_b)
    assert a.shape == (n_a, 8) and b.shape == (n_b, 8) and k == 5
    assert sorted(set(ref["radii_a"].tolist())) == sorted(set(ref["radii_b"].tolist())) == list(cases.RAMP_RADII)
    assert ref["ties"] == cases.RAMP_TIES == 8296
    assert ref["counts"].tolist() == cases.RAMP_COUNTS[(n_a, n_b)]
    assert cases.RAMP_COUNTS == {(2100, 2077): [2077, 2081, 6235, 2078], (2077, 2100): [2081, 2077, 6245, 2077]}
    assert ref["min_gap"] >= MIN_GAP
    # exact small integers: the Gram form gives the same numbers to the bit, whatever the summation order
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    g = a64 @ b64.T
    d2 = (a64 * a64).sum(axis=1)[:, None] + (b64 * b64).sum(axis=1)[None, :] - 2.0 * g
    i, j = np.arange(n_a)[:, None], np.arange(n_b)[None, :]
    assert np.array_equal(d2, 5.0 * (i - j) ** 2 + 25.0) and d2.max() < 2.0 ** 53
