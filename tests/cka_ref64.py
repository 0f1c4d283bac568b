"""The yardstick for layer-wise CKA (include/dt_hip_cka.h), in plain numpy.

Every sum is taken in ``np.longdouble`` (x87 extended: unit roundoff 2^-64, 2048 times below fp64's), with one
exception that is part of the contract and not of the arithmetic under test: the column means.  The header DEFINES them
as the fp64 sum over the rows in the order i = 0 .. n-1 followed by one division, so ``column_means`` forms exactly that
float64 number (bit for bit what the device forms), and everything after it -- centring, Gram, both estimators -- is
extended precision.  Both estimators are invariant to a shift of the features (tests/test_cka_host.py checks it), so
which nearby mean is subtracted does not move a score beyond rounding; it only fixes which Gram the cells are compared
with.  This is a deviation from "every sum in extended precision", and it makes ``centred_gram`` depend on one step of the
algorithm under test; ``exact_centred_gram`` is the fully independent reference (exact means), and
``exact_mean_cell_bound`` the cell tolerance against it, with the rounding of the contract's mean as an extra term.

``forward_bound`` is the a-priori tolerance for a device score, derived below from the number formats, never from what
the device returns.
"""
import itertools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53                     # unit roundoff of fp64
SLAB = 1024                        # DT_CKA_SLAB
NONFINITE, ZERO_VARIANCE, SELF_NOT_POSITIVE = 1, 2, 4


def column_means(X):
    """float64: the rows added in order, then one division (the contract's definition)"""
    X = np.asarray(X, dtype=np.float32)
    s = np.zeros(X.shape[1], dtype=np.float64)
    for row in X:
        s += row.astype(np.float64)
    return s / np.float64(X.shape[0])


def centred(X, means=None):
    """[n, p] longdouble: X minus the contract's means (or minus ``means``)"""
    X = np.asarray(X, dtype=np.float32).reshape(len(X), -1)
    m = column_means(X) if means is None else means
    return X.astype(LD) - np.asarray(m).astype(LD)


def gram(Xc):
    Xc = np.asarray(Xc, dtype=LD)
    return Xc @ Xc.T


def centred_gram(X):
    """K' of the header for a layer [n, ...] of float32"""
    return gram(centred(X))


def centre_gram(K):
    """H K H with H = I - 11'/n"""
    K = np.asarray(K, dtype=LD)
    n = K.shape[0]
    H = np.eye(n, dtype=LD) - np.ones((n, n), dtype=LD) / LD(n)
    return H @ K @ H


def inner(K, L):
    return (np.asarray(K, dtype=LD) * np.asarray(L, dtype=LD)).sum()


def cka_biased(K, L):
    """<K, L> / sqrt(<K, K> <L, L>) for Grams that are centred already"""
    return inner(K, L) / np.sqrt(inner(K, K) * inner(L, L))


def off_diagonal(K):
    K = np.array(K, dtype=LD)
    np.fill_diagonal(K, 0)
    return K


def hsic1(K, L, dtype=LD):
    """Song et al. (2012), eq. 5, as Nguyen, Raghu and Kornblith (2021) use it, the operations in the header's order
    (``dtype=np.float64``: the device's own arithmetic, exact and so order-free wherever every sum is)"""
    Kt, Lt = off_diagonal(K).astype(dtype), off_diagonal(L).astype(dtype)
    n = dtype(Kt.shape[0])
    rk, rl = Kt.sum(axis=1), Lt.sum(axis=1)
    c1 = (rk.sum() * rl.sum()) / ((n - 1) * (n - 2))
    c2 = (2 * (rk * rl).sum()) / (n - 2)
    return (((Kt * Lt).sum() + c1) - c2) / (n * (n - 3))


def hsic1_brute_force(K, L):
    """The fourth-order U-statistic itself: the mean over all ordered 4-tuples of distinct indices of
    K_ij L_ij + K_ij L_qr - 2 K_ij L_iq.  n <= 7 or so."""
    K, L = np.asarray(K, dtype=LD), np.asarray(L, dtype=LD)
    n = K.shape[0]
    total, count = LD(0), 0
    for i, j, q, r in itertools.permutations(range(n), 4):
        total += K[i, j] * L[i, j] + K[i, j] * L[q, r] - 2 * K[i, j] * L[i, q]
        count += 1
    return total / count


def cka_unbiased(K, L):
    return hsic1(K, L) / np.sqrt(hsic1(K, K) * hsic1(L, L))


def status(X, K=None):
    """the status word of the header for a layer"""
    X = np.asarray(X, dtype=np.float32).reshape(len(X), -1)
    if not np.isfinite(X).all():
        return NONFINITE
    K = centred_gram(X) if K is None else K
    if inner(K, K) == 0:
        return ZERO_VARIANCE
    return 0 if hsic1(K, K) > 0 else SELF_NOT_POSITIVE


def scores(layers_a, layers_b):
    """dict(cka, cka_unbiased [La, Lb] longdouble (NaN where the header says so), status_a, status_b, grams_a, grams_b)"""
    def side(layers):
        layers = [np.asarray(X, dtype=np.float32).reshape(len(X), -1) for X in layers]
        st = [status(X) for X in layers]
        grams = [centred_gram(X) if s != NONFINITE else np.full((len(X), len(X)), np.nan, dtype=LD) for X, s in zip(layers, st)]
        return grams, np.array(st)
    (Ka, sa), (Kb, sb) = side(layers_a), side(layers_b)
    cka = np.full((len(Ka), len(Kb)), np.nan, dtype=LD)
    unb = cka.copy()
    for i, j in itertools.product(range(len(Ka)), range(len(Kb))):
        if not (sa[i] | sb[j]) & (NONFINITE | ZERO_VARIANCE):
            cka[i, j] = cka_biased(Ka[i], Kb[j])
        if not sa[i] | sb[j]:
            unb[i, j] = cka_unbiased(Ka[i], Kb[j])
    return dict(cka=cka, cka_unbiased=unb, status_a=sa, status_b=sb, grams_a=Ka, grams_b=Kb)


# ------------------------------------------------------------------------------------------------ tolerances
def gamma(p, n):
    """A device Gram cell is p fused multiply-adds in slabs, the slabs added in turn, on values that each carry one
    rounding of x - m: at most p + p / SLAB + 2 roundings, each of relative size U on a partial sum that Cauchy-Schwarz
    bounds by |x_i - m| |x_j - m|.  (p + n + 8) U covers that for every p (p / SLAB + 2 <= n + 8 holds up to p = 10 SLAB at
    n = 4 and further for larger n: the test widths end at 2 SLAB + 5) and leaves the n + 8 for the n-long chains
    and 8-deep trees of the score stage."""
    return (p + n + 8) * U


def cell_bound(X):
    """[n, n] float64: gamma |x_i - m| |x_j - m|, the tolerance of the cells of a layer's device Gram"""
    Xc = centred(X)
    norms = np.sqrt((Xc * Xc).sum(axis=1))
    return (gamma(Xc.shape[1], Xc.shape[0]) * np.outer(norms, norms)).astype(np.float64)


def exact_centred_gram(X):
    """the Gram about the EXACT column means (extended precision throughout): independent of the contract's mean"""
    Xl = np.asarray(X, dtype=np.float32).reshape(len(X), -1).astype(LD)
    return gram(Xl - Xl.sum(axis=0) / LD(Xl.shape[0]))


def exact_mean_cell_bound(X):
    """Tolerance of a device cell against ``exact_centred_gram``.  The contract's mean m differs from the exact one by
    d_k with |d_k| <= U sum_i |x_ik| (n - 1 roundings of partial sums that never exceed sum_i |x_ik|, and one of the
    division, over n).  Centring about m + d instead of m moves cell (i, j) by -d.(x_i - m) - d.(x_j - m) + |d|^2, so the
    cell bound grows by |d| (|x_i - m| + |x_j - m|) + |d|^2 with |d| bounded as above."""
    Xf = np.asarray(X, dtype=np.float32).reshape(len(X), -1)
    Xc = centred(Xf)
    norms = np.sqrt((Xc * Xc).sum(axis=1)).astype(np.float64)
    d = U * np.sqrt((np.abs(Xf.astype(np.float64)).sum(axis=0) ** 2).sum())
    return cell_bound(Xf) + d * np.add.outer(norms, norms) + d * d


def kappa(K):
    """tr K' / |K'|_F <= sqrt(n).  The cell errors above add up to a Frobenius error of at most gamma tr K' (the
    square root of sum_ij |x_i|^2 |x_j|^2), that is gamma kappa relative to |K'|_F."""
    return float(np.trace(K) / np.sqrt(inner(K, K)))


def rho(K):
    """|K'|_F^2 / (n (n - 3) HSIC1(K, K)): how much smaller the debiased self term is than the biased one, and so how
    much larger a relative error of the Gram appears in it"""
    n = K.shape[0]
    return float(inner(K, K) / (n * (n - 3) * hsic1(K, K)))


def forward_bound(layers_a, layers_b):
    """(bound of cka, bound of cka_unbiased), [La, Lb] float64 each.
    cka = <K, L> / (|K| |L|): a relative Frobenius error e_K of K and e_L of L moves it by at most 2 (e_K + e_L) to first
    order (numerator e_K + e_L, denominator the same); with e = gamma kappa and a factor 2 for the second order and the
    score stage's own roundings (kappa >= 1, so the margin is at least 4 gamma > 4 (n + 8) U): 4 gamma (kappa_K + kappa_L).
    The debiased score is the same expression in HSIC1 terms, whose size is 1 / rho of the biased ones while the
    absolute errors stay: the bound times max(rho_K, rho_L)."""
    Ka, Kb = [centred_gram(X) for X in layers_a], [centred_gram(X) for X in layers_b]
    n = Ka[0].shape[0]
    width = lambda X: int(np.prod(np.shape(X)[1:]))
    g = gamma(max(width(X) for X in list(layers_a) + list(layers_b)), n)
    biased = np.array([[4 * g * (kappa(K) + kappa(L)) for L in Kb] for K in Ka])
    worst = np.array([[max(rho(K), rho(L)) for L in Kb] for K in Ka])
    return biased, biased * worst


def nonpositive_self_layer(n=4, tries=200, seed=0):
    """A layer [n, n] with HSIC1(K, K) <= 0 and <K', K'> > 0, from a seeded search over 0/1 layers.  The debiased self
    term is a U-statistic, not a norm: for a feature-centred Gram it vanishes, for instance, on one-hot layers
    (K' = I - 11'/n), and random real-valued layers [4, p] stay above zero (5000 draws: never below 1e-5 <K', K'>), so
    the search runs where the arithmetic is exact.  With n a power of two every mean, centred value, cell and sum of such
    a layer is a dyadic rational that fp64 holds exactly, so the sign the device sees is the sign found here: the layer is
    accepted when the header's formula in float64 gives <= 0.  Returns (X float32, that value)."""
    rs = np.random.RandomState(seed)
    for _ in range(tries):
        X = rs.randint(0, 2, size=(n, n)).astype(np.float32)
        K = centred_gram(X)
        h = hsic1(K, K, np.float64)
        if inner(K, K) > 0 and h <= 0 and hsic1(K, K) <= 0:
            return X, float(h)
    raise AssertionError(f"no 0/1 layer [{n}, {n}] with HSIC1(K, K) <= 0 in {tries} seeded draws")
