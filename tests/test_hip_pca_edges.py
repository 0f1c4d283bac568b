"""GPU: the device PCA (include/dt_hip_pca.h) against the float64 yardstick at the edges of its eigen stage: repeated
eigenvalues, a tridiagonal that splits, a rank below k, n = 2 .. 4, k = 1, k = n - 1, k = E = 4, a common offset far above
the variation, rows scaled by 2^40 and 2^-40.  The cases and the comparers, which do not assume a unique basis, are in
tests/pca_cases.py; tests/test_pca_host.py guards both without a GPU.  A null direction (include/dt_hip_pca.h) is all
zeros.  Each test prints the figures it asserts on."""
import functools
import warnings

import numpy as np
import pytest
import torch

from distillation_trajectories_amd import engine
from distillation_trajectories_amd.analysis.dimensionality.pca import TrajectoryPCA
import pca_cases as pc

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
FIELDS = ("mean", "components", "scores", "singular_values", "explained_variance", "explained_variance_ratio")


def _sets(name, split=None):
    """the case's rows on the device: (a, b) with b None for one set"""
    c = pc.case(name)
    rows = torch.from_numpy(c["rows"].copy()).to(DEV)
    split = c["split"] if split is None else split
    return (rows, None) if not split else (rows[:split].contiguous(), rows[split:].contiguous())


@functools.lru_cache(maxsize=None)
def _fit(name):
    a, b = _sets(name)
    return engine.device_pca(a, pc.case(name)["k"], b)


def _answer(r, p=0):
    return {f: r[f][p].cpu().numpy() for f in FIELDS}


def _same_bits(r, p, s, q, what):
    for f in FIELDS + ("status",):
        assert torch.equal(r[f][p], s[f][q]), (what, f)


@pytest.mark.parametrize("name", pc.CASES)
def test_case_matches_ref64(name):
    c = pc.case(name)
    r = _fit(name)
    assert r["status"].cpu().tolist() == [0]
    got = _answer(r)
    dead = pc.null_directions(c["ref"], c["k"])
    print(f"{name}: singular values {got['singular_values']}, null directions {dead}, largest |component| there "
          f"{[float(np.abs(got['components'][j]).max()) for j in dead]}")
    fig = pc.compare(got, c["rows"], c["ref"], c["k"], name)
    print(f"{name}: " + ", ".join(f"{key} {value:.2e}" for key, value in fig.items()))
    if name in pc.SEPARATED:
        pc.compare_vectors(got, c["ref"], c["k"], name)


@pytest.mark.parametrize("name,split", [("n2_split", 1), ("three_points", 7)])
def test_two_sets_equal_one_stacked_set(name, split):
    k = pc.case(name)["k"]
    a, b = _sets(name, split)
    assert b is not None and len(a) == split
    two, one = engine.device_pca(a, k, b), engine.device_pca(torch.cat([a, b]), k)
    _same_bits(two, 0, one, 0, name)
    if pc.case(name)["split"] == split:
        _same_bits(two, 0, _fit(name), 0, name)


def test_batch_of_repeated_null_and_full_rank_problems():
    """pairs12 (a double eigenvalue), rank1 (two null directions) and a walk in one call: each problem has the bits it has
    alone, wherever it stands in the batch"""
    k = 3
    rows = {name: torch.from_numpy(pc.case(name)["rows"].copy()).to(DEV) for name in pc.BATCH}
    alone = {name: engine.device_pca(rows[name], k) for name in pc.BATCH}
    for order in (pc.BATCH, pc.BATCH[::-1], (pc.BATCH[2], pc.BATCH[0], pc.BATCH[1])):
        r = engine.device_pca(torch.stack([rows[name] for name in order], dim=1), k)
        assert r["status"].cpu().tolist() == [0, 0, 0]
        for p, name in enumerate(order):
            _same_bits(r, p, alone[name], 0, (order, name))
    for name in pc.BATCH:
        c = pc.case(name)
        fig = pc.compare(_answer(alone[name]), c["rows"], c["ref"], k, name)
        print(f"{name}: " + ", ".join(f"{key} {value:.2e}" for key, value in fig.items()))


@pytest.mark.parametrize("name", pc.CASES)
def test_projection_reproduces_the_scores(name):
    c = pc.case(name)
    r = _fit(name)
    a, b = _sets(name)
    proj = engine.device_pca_project(a, r["mean"][0], r["components"][0], b)[0].cpu().numpy()
    scores = r["scores"][0].cpu().numpy()
    off = np.abs(proj.astype(np.float64) - scores).max() / np.abs(scores).max()
    print(f"{name}: projection against scores {off:.2e}")
    assert off <= 1e-6, (name, off)
    for j in pc.null_directions(c["ref"], c["k"]):
        assert not proj[:, j].any() and not scores[:, j].any(), (name, j)


@pytest.mark.parametrize("name", ["pairs", "three_points"])
def test_trajectory_pca_on_numpy_rows(name):
    c = pc.case(name)
    r = _fit(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pca = TrajectoryPCA(c["k"])
        scores = pca.fit_transform(c["rows"].copy())
    assert isinstance(scores, np.ndarray)
    assert np.array_equal(scores, r["scores"][0].cpu().numpy())
    assert np.array_equal(pca.components_, r["components"][0].cpu().numpy())
    assert np.array_equal(pca.singular_values_, r["singular_values"][0].cpu().numpy())
    assert np.array_equal(pca.explained_variance_ratio_, r["explained_variance_ratio"][0].cpu().numpy())
