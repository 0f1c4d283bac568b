"""The seeded feature sets that tests/test_cka_host.py and tests/test_hip_cka.py share, and the yardstick's results on
them (tests/cka_ref64.py), each computed once per process and never changed afterwards.

A case is two lists of layers over the same n inputs.  A layer [n, p] is a shared low-rank signal Z [n, rank] (one Z per
case, so that the layers of both sides represent the same thing) through a random map of its own, plus white noise, plus
an offset of its own per feature, rounded to fp32.  ``independent`` has no signal: its debiased score is meant to be
near zero while the biased one is not.
"""
import functools

import numpy as np

import cka_ref64 as ref

SLAB = ref.SLAB
# name -> (seed, n, widths of side a, widths of side b, rank of the signal (0: none), noise)
CASES = {
    "small": (11, 12, (3, 17, 64), (5, 40), 3, 0.3),
    "slabs": (12, 37, (SLAB - 1, SLAB), (SLAB + 1, 2 * SLAB + 5, 130), 4, 0.5),
    "tiles": (13, 130, (48, 300), (33,), 6, 0.5),
    "independent": (14, 16, (200,), (200,), 0, 1.0),
}
NEAR_ZERO = ("independent",)


def layer(rs, Z, p, noise):
    n = Z.shape[0]
    X = noise * rs.standard_normal((n, p))
    if Z.shape[1]:
        X = X + Z @ rs.standard_normal((Z.shape[1], p))
    return (X + rs.uniform(-2.0, 2.0, size=p)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(a, b: lists of float32 layers [n, p]; ref: cka_ref64.scores; bound: cka_ref64.forward_bound), read-only"""
    seed, n, wa, wb, rank, noise = CASES[name]
    rs = np.random.RandomState(seed)
    Z = rs.standard_normal((n, rank))
    a = [layer(rs, Z, p, noise) for p in wa]
    b = [layer(rs, Z, p, noise) for p in wb]
    for X in a + b:
        X.setflags(write=False)
    return dict(a=a, b=b, n=n, ref=ref.scores(a, b), bound=ref.forward_bound(a, b))
