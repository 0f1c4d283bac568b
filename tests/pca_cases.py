"""The edge cases of the device PCA that tests/test_pca_host.py and tests/test_hip_pca_edges.py share, the yardstick's
result on each (tests/pca_ref64.py), and the comparers that do not assume a unique basis.  Every case is built once per
process and is read-only afterwards.

A case is fp32 rows [n, E] and a k.  The "exact" ones are small integers, so that rows, means and the centred Gram matrix
G are exact in fp64 and the spectrum of G is the stated one (``identity`` is the exception: its mean 1/12 rounds, so its
eleven eigenvalues are 1 to a few ulps).

  n2, n2_split     seeded walk, n = 2: no tridiagonalisation step (n2_split: one row in each set)
  n3, n4           seeded walk, k = n - 1: one and two steps
  e4               40 x 4, k = E = 4: one quad per row, n > E + 1
  k1               20 x 16, k = 1
  offset           walk with steps of 1e-2 around 1e4: passes only because G is centred before the product
  pairs            exact: 7 +- a, 7 +- b, 7 +- c on disjoint supports, |a|^2 = |b|^2 = 15, |c|^2 = 4: lambda = 30, 30, 8, 0, 0;
                   G is block diagonal, so every reflector has tau = 0 and the tridiagonal splits
  stalled          exact: m, m, m +- a, m +- b, m +- c: the same spectrum, and two centred rows are exactly zero, so the
                   first reflector has tau = 0 and e[0] = 0
  identity_k4/k11  the rows of the 12 x 12 identity: lambda = 1 eleven times, then 0; with k = 4 the subspace is not unique
  rank1            exact: t_i a + 3 for t = 0 .. 11 and an integer a: rank 1 below k = 3
  three_points     exact: 15 states cycling through 3 integer points whose centroid is an integer point: rank 2 below k = 4
  near             24 x 16 with lambda in proportion 1, 1 - 1e-5, 1 - 2e-5, 0.25, 0.01, 1e-4: gaps inside the kernel's
                   cluster rule (1e-3 of the tridiagonal's norm), yet a well-conditioned problem
  big, small       seeded walk times 2^40 and 2^-40
  pairs12, walk12  the batch's partners of rank1 (n = 12, E = 16, k = 3): ``pairs`` with every row twice, and a walk

A walk has the suite's usual offset of 5.0.  ``offset`` is nudged by at most one fp32 ulp per entry so that each column
mean is itself an fp32 number: the library's fp32 ``mean`` is then exact, and the two bounds that go through it (consistency
here, the projection in the GPU test) apply as they stand.  With a rounded mean of 1e4 they could not: half an ulp of 1e4 is
4.9e-4, against scores of about 0.1.
"""
import functools

import numpy as np

from pca_ref64 import ambiguous_sign, pca_ref64

CLUSTER = 1e-3     # reference eigenvalues within CLUSTER * lambda_0 of each other are one cluster
GAP = 1e-2         # every cluster of a wanted eigenvalue is at least GAP * lambda_0 away from everything else
NULL = 1e-12       # a direction with lambda_j <= NULL * lambda_0 in the reference is null
FLOOR = 1e-5       # no wanted eigenvalue lies between the two: above NULL means above FLOOR * lambda_0

A = (3, 2, 1, 1)
B = (1, -2, 3, 1)
C = (0, 2, 0, 0)
RANK1_A = (1, -2, 3, 0, 2, -1, 1, 4, 0, -3, 2, 1, -1, 2, 0, 1)
NEAR_LAMBDA = (1.0, 1.0 - 1e-5, 1.0 - 2e-5, 0.25, 0.01, 1e-4)


def walk(seed, n, E, step=1.0, offset=5.0, scale=1.0):
    rs = np.random.RandomState(seed)
    return ((rs.standard_normal((n, E)).cumsum(0) * step + offset) * scale).astype(np.float32)


def _offset(seed, n, E):
    X = walk(seed, n, E, step=1e-2, offset=1e4)
    q = 2.0 ** -10                                            # the fp32 ulp in [8192, 16384)
    m = np.round(X.astype(np.float64) / q).astype(np.int64)
    assert np.array_equal(m * q, X.astype(np.float64))
    for e in range(E):
        m[:m[:, e].sum() % n, e] -= 1                         # now the column sum is a multiple of n
    X = (m * q).astype(np.float32)
    assert X.min() >= 8192 and X.max() < 16384
    return X


def _signed(base, vectors):
    """rows base + v, base - v for each v (each v on its own four columns of E = 16)"""
    rows = []
    for i, v in enumerate(vectors):
        full = np.zeros(16)
        full[4 * i:4 * i + 4] = v
        rows += [base + full, base - full]
    return rows


def _pairs(repeat=1):
    return np.array(_signed(np.full(16, 7.0), (A, B, C)) * repeat, dtype=np.float32)


def _stalled():
    m = np.arange(16) % 5 + 2.0
    return np.array([m, m] + _signed(m, (A, B, C)), dtype=np.float32)


def _rank1():
    return (np.arange(12.0)[:, None] * np.array(RANK1_A, dtype=np.float64) + 3.0).astype(np.float32)


def _three_points():
    rs = np.random.RandomState(41)
    centre, p0, p1 = rs.randint(-4, 5, (3, 16)).astype(np.float64)
    points = [centre + p0, centre + p1, centre - p0 - p1]
    return np.array([points[i % 3] for i in range(15)], dtype=np.float32)


def _near():
    rs = np.random.RandomState(42)
    U = np.linalg.qr(np.hstack([np.ones((24, 1)), rs.standard_normal((24, 6))]))[0][:, 1:]     # columns sum to zero
    V = np.linalg.qr(rs.standard_normal((16, 6)))[0]
    return ((U * (8.0 * np.sqrt(NEAR_LAMBDA))) @ V.T + 0.5).astype(np.float32)


# name -> (rows, k, rows in the first set when the case is given as two sets)
BUILDERS = {
    "n2": (lambda: walk(101, 2, 8), 1, None),
    "n2_split": (lambda: walk(102, 2, 8), 1, 1),
    "n3": (lambda: walk(103, 3, 8), 2, None),
    "n4": (lambda: walk(104, 4, 8), 3, None),
    "e4": (lambda: walk(105, 40, 4), 4, None),
    "k1": (lambda: walk(106, 20, 16), 1, None),
    "offset": (lambda: _offset(107, 30, 16), 3, None),
    "pairs": (_pairs, 3, None),
    "stalled": (_stalled, 3, None),
    "identity_k4": (lambda: np.eye(12, dtype=np.float32), 4, None),
    "identity_k11": (lambda: np.eye(12, dtype=np.float32), 11, None),
    "rank1": (_rank1, 3, None),
    "three_points": (_three_points, 4, None),
    "near": (_near, 4, None),
    "big": (lambda: walk(108, 20, 16, scale=2.0 ** 40), 3, None),
    "small": (lambda: walk(109, 20, 16, scale=2.0 ** -40), 3, None),
    "pairs12": (lambda: _pairs(2), 3, None),
    "walk12": (lambda: walk(110, 12, 16), 3, None),
}
CASES = tuple(name for name in BUILDERS if name not in ("pairs12", "walk12"))
SEPARATED = ("offset", "big", "small")            # also through the vector-against-vector comparison
BATCH = ("pairs12", "rank1", "walk12")            # one call with P = 3
# the leading eigenvalues of G that a case states
STATED = {"pairs": (30, 30, 8, 0, 0), "stalled": (30, 30, 8, 0, 0), "pairs12": (60, 60, 16, 0, 0),
          "identity_k4": (1,) * 11 + (0,), "identity_k11": (1,) * 11 + (0,),
          "rank1": (143 * sum(a * a for a in RANK1_A), 0, 0)}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(rows [n, E] fp32, k, split (rows in set a when run as two sets, or None), ref: pca_ref64 of the rows)"""
    build, k, split = BUILDERS[name]
    rows = build()
    rows.setflags(write=False)
    ref = pca_ref64(rows, k)
    for v in ref.values():
        v.setflags(write=False)
    return dict(name=name, rows=rows, k=k, split=split, ref=ref)


# ---------------------------------------------------------------------------------------------- structure of a spectrum
def spectrum(ref):
    """the reference's eigenvalues of G, descending, with the 0 that a centred G always has appended"""
    return np.append(ref["spectrum"], 0.0)


def clusters(lam):
    """lists of indices: neighbours in the descending spectrum within CLUSTER * lambda_0 of each other share a cluster"""
    out = [[0]]
    for i in range(1, len(lam)):
        if lam[i - 1] - lam[i] <= CLUSTER * lam[0]:
            out[-1].append(i)
        else:
            out.append([i])
    return out


def null_directions(ref, k):
    lam = ref["spectrum"]
    return [j for j in range(k) if lam[j] <= NULL * lam[0]]


def check_preconditions(ref, k):
    """what lets the comparers tell a cluster from a gap and a null direction from a small one without tuning"""
    lam = spectrum(ref)
    assert lam[0] > 0
    for members in clusters(lam):
        wanted = [j for j in members if j < k and lam[j] > NULL * lam[0]]
        if not wanted:
            continue
        assert lam[members[0]] - lam[members[-1]] <= CLUSTER * lam[0], ("a chain wider than a cluster", members)
        if members[0] > 0:
            assert lam[members[0] - 1] - lam[members[0]] >= GAP * lam[0], ("gap above", members)
        assert lam[members[-1]] - lam[members[-1] + 1] >= GAP * lam[0], ("gap below", members)
        assert lam[wanted[-1]] >= FLOOR * lam[0], ("a wanted eigenvalue between null and small", wanted)


# ---------------------------------------------------------------------------------------------- comparers
def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-30)


def compare_vectors(got, ref, k, what):
    """scores / components / mean to 2e-6 of each vector's max-abs; singular values and variances to 1e-9 relative.  A
    component whose two largest |entries| are within 1e-6 with opposite signs may carry either sign (svd_flip's choice
    then rests on rounding).  For separated spectra only."""
    assert close(got["mean"], ref["mean"], 2e-6), what
    for name in ("singular_values", "explained_variance", "explained_variance_ratio"):
        assert close(got[name], ref[name], 1e-9), (what, name, got[name], ref[name])
    for j in range(k):
        c, s = np.asarray(got["components"][j], np.float64), np.asarray(got["scores"][:, j], np.float64)
        rc, rs = ref["components"][j], ref["scores"][:, j]
        if ambiguous_sign(rc) and not close(c, rc, 2e-6):
            c, s = -c, -s
        assert close(c, rc, 2e-6), (what, j, np.abs(c - rc).max())
        assert close(s, rs, 2e-6), (what, j, np.abs(s - rs).max())


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def compare(got, rows, ref, k, what=""):
    """A PCA answer (the six fields of the library, numpy) against the reference, without assuming a unique basis.
    Returns the worst figure of each bound: dict(variance, containment, orthonormality, consistency).

    - mean to 2e-6, explained variance and ratio to 1e-9 of the vector's max-abs;
    - singular values: sqrt(explained_variance (n - 1)) of the answer itself to 1e-15 relative, and the reference's to 1e-9
      at the non-null directions (a Gram-based route cannot resolve a singular value below sqrt(n eps) s_0);
    - a null direction (lambda_j <= 1e-12 lambda_0 in the reference): singular value, variance, ratio, component and score
      column are exactly zero;
    - a non-null component: containment in the span of the reference's whole cluster, max|c - V^T V c| <= 2e-6 max|c|;
      consistency, scores[:, j] = (rows - mean) c_j in float64 from the answer's own mean and component, to 2e-6 of the
      largest |score| (a rounded mean shifts every column by the same absolute amount, so the bound is the matrix's, as in
      the projection test); alone in its cluster, component and score column against the reference's to 2e-6 as
      ``compare_vectors`` does, sign included; in a repeated cluster, the sign rule on the component itself;
    - the non-null components together: |C C^T - I| <= 5e-7.
    """
    n = rows.shape[0]
    g = {f: np.asarray(got[f], np.float64) for f in ("mean", "components", "scores", "singular_values",
                                                       "explained_variance", "explained_variance_ratio")}
    lam = spectrum(ref)
    fig = dict(variance=0.0, containment=0.0, orthonormality=0.0, consistency=0.0)
    assert close(g["mean"], ref["mean"], 2e-6), (what, "mean")
    for name in ("explained_variance", "explained_variance_ratio"):
        fig["variance"] = max(fig["variance"], _rel(g[name], ref[name]))
        assert close(g[name], ref[name], 1e-9), (what, name, g[name], ref[name])
    sv, own = g["singular_values"], np.sqrt(g["explained_variance"] * (n - 1))
    assert np.all(np.abs(sv - own) <= 1e-15 * own), (what, "singular values against the answer's own variance", sv, own)
    dead = null_directions(ref, k)
    live = [j for j in range(k) if j not in dead]
    fig["variance"] = max(fig["variance"], _rel(sv[live], ref["singular_values"][live]))
    assert close(sv[live], ref["singular_values"][live], 1e-9), (what, "singular values", sv, ref["singular_values"])
    for j in dead:
        values = (sv[j], g["explained_variance"][j], g["explained_variance_ratio"][j])
        assert values == (0.0, 0.0, 0.0), (what, "null direction", j, values)
        assert not g["components"][j].any(), (what, "null direction", j, "component", np.abs(g["components"][j]).max())
        assert not g["scores"][:, j].any(), (what, "null direction", j, "scores", np.abs(g["scores"][:, j]).max())
    centred = rows.astype(np.float64) - g["mean"]
    top = np.abs(g["scores"]).max()
    for members in clusters(lam):
        for j in (j for j in members if j in live):
            c, s = g["components"][j], g["scores"][:, j]
            V = ref["basis"][[i for i in members if i < len(ref["basis"])]]
            out = np.abs(c - V.T @ (V @ c)).max() / np.abs(c).max()
            fig["containment"] = max(fig["containment"], out)
            assert out <= 2e-6, (what, "containment", j, out)
            off = np.abs(s - centred @ c).max() / top
            fig["consistency"] = max(fig["consistency"], off)
            assert off <= 2e-6, (what, "consistency", j, off)
            if len(members) == 1:
                rc, rs = ref["components"][j], ref["scores"][:, j]
                if ambiguous_sign(rc) and not close(c, rc, 2e-6):
                    c, s = -c, -s
                assert close(c, rc, 2e-6), (what, "component", j, np.abs(c - rc).max())
                assert close(s, rs, 2e-6), (what, "score column", j, np.abs(s - rs).max())
            else:
                assert c[np.argmax(np.abs(c))] > 0, (what, "sign rule", j)
    Cl = g["components"][live]
    fig["orthonormality"] = np.abs(Cl @ Cl.T - np.eye(len(live))).max()
    assert fig["orthonormality"] <= 5e-7, (what, "orthonormality", fig["orthonormality"])
    return fig


def reference_answer(ref, k):
    """the reference's answer in the library's fields, null directions as the library reports them: zeros"""
    out = {f: np.array(ref[f]) for f in ("mean", "components", "scores", "singular_values", "explained_variance",
                                         "explained_variance_ratio")}
    for j in null_directions(ref, k):
        for f in ("singular_values", "explained_variance", "explained_variance_ratio"):
            out[f][j] = 0.0
        out["components"][j] = 0.0
        out["scores"][:, j] = 0.0
    return out
