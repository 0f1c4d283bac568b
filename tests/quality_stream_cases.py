"""The cases of the row-panel route of the device sample-quality scores (include/dt_hip_quality_stream.h,
tests/test_hip_quality_stream.py), scored by the float64 yardstick quality_ref64, which this module imports and does not
change.  tests/test_quality_stream_host.py checks the gap precondition of every case without a GPU."""
import functools

import numpy as np

import quality_ref64 as q

# name -> (n_a, n_b, P, D, k); the teacher (set A) is shared by the P problems of a case
SHAPES = {
    "2049x2049_D64": (2049, 2049, 1, 64, 5),             # one row past the old limit and past the LDS buffer
    "4100x2100_P4_D128": (4100, 2100, 4, 128, 3),        # several panels and refills, a ragged last tile, four modes
    "2100x4161_D36_k63": (2100, 4161, 1, 36, 63),        # D no multiple of 16
    "2111x2065_D2048": (2111, 2065, 1, 2048, 5),
    "130x70_D2048": (130, 70, 1, 2048, 5),               # well below the old limit
    "2100x2090_D16_k1023": (2100, 2090, 1, 16, 1023),    # the largest k
}
# the seed of a case's pool is 7000 + 13 n_a + n_b + D unless it is listed here.  The k = 1023 case keeps the rule's seed
# (36406): its pool decides every comparison by far more than the 100 bounds the tests ask for
# (tests/test_quality_stream_host.py prints the figure).
SEEDS = {"2100x2090_D16_k1023": 36406}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(a, [b_0 .. b_P-1], k, [quality_ref64 of (a, b_p)]) of a case, the problems made as quality_ref64.shape_case makes
    them: problem 0 is the pooled pair as it is, the others go through "shift", "collapse" and "spread" in turn"""
    n_a, n_b, P, D, k = SHAPES[name]
    seed = SEEDS.get(name, 7000 + 13 * n_a + n_b + D)
    pairs = [q.feature_pair(seed, n_a, n_b, D, q.MODES[0 if p == 0 else 1 + (p - 1) % 3], 0 if p == 0 else (p - 1) // 3)
             for p in range(P)]
    a = pairs[0][0]
    assert all(np.array_equal(a, x) for x, _ in pairs)
    bs = [y for _, y in pairs]
    return a, bs, k, [q.quality_ref64(a, y, k) for y in bs]


RAMPS = ((2100, 2077), (2077, 2100))
RAMP_K = 5
RAMP_RADII = (45.0, 80.0, 125.0)
RAMP_TIES = 8296
RAMP_COUNTS = {(2100, 2077): [2077, 2081, 6235, 2078], (2077, 2100): [2081, 2077, 6245, 2077]}


@functools.lru_cache(maxsize=None)
def ramp(n_a, n_b):
    """(a, b, k, quality_ref64(a, b, k, form="direct")): D = 8, a_i = i (1, 2, 0, ...), b_j = j (1, 2, 0, ...) +
    (0, 0, 3, 4, 0, ...).  Every quantity is a small integer, exact in fp64 in any summation order: d2(a_i, a_j) =
    5 (i - j)^2, d2(a_i, b_j) = 5 (i - j)^2 + 25, radii 45 inside and 80, 125 at the two ends, and exact ties between d2 and
    r2 that strict < must not count.  Row 0 sees its distances ascending (the selection's threshold drops everything
    after the first refill), the last row sees them descending (every key passes the threshold), with duplicate values
    at the radius."""
    D = 8
    a, b = np.zeros((n_a, D), np.float32), np.zeros((n_b, D), np.float32)
    a[:, 0], a[:, 1] = np.arange(n_a), 2 * np.arange(n_a)
    b[:, 0], b[:, 1] = np.arange(n_b), 2 * np.arange(n_b)
    b[:, 2], b[:, 3] = 3.0, 4.0
    return a, b, RAMP_K, q.quality_ref64(a, b, RAMP_K, form="direct")
