"""The yardstick for the entropic transport cost (include/dt_hip_sinkhorn.h), in plain numpy.

The header's iteration in ``np.longdouble`` (x87 extended: unit roundoff 2^-64, 2048 times below fp64's): the cost matrix
from differences, g = 0, per step f_i = -eps (LSE_j((g_j - C_ij) / eps) - log n_b), g'_j = -eps (LSE_i((f_i - C_ij) / eps)
- log n_a), err = mean_j |expm1((g_j - g'_j) / eps)|, g = g', the same stopping rule, ot = mean f + mean g.

``forward_bound`` is the a-priori tolerance for a device output, derived from the number formats, never from what the
device returns.  With u = 2^-53:

  * cost: d = double(a) - double(b) is exact, the chain of E fused multiply-adds of non-negative terms is within E u c
    (1 + O(E u)) of c: |dC_ij| <= (E + 1) u c_ij.  For p = 1 the square root halves the relative error and rounds once:
    |dC_ij| <= ((E + 1) / 2 + 1) u C_ij.  dC is the largest of them.
  * the soft-min map (g, C) -> f is non-expansive in the max norm in both arguments, so after K steps (2K half-steps)
        |f - f_ref|, |g - g_ref| <= e_K = 2 K (dC + d_step),
    d_step the rounding of one half-step.  In units of u and of the exponent (multiply by eps for a potential), with
    Z = max |z| over all steps and n = max(n_a, n_b):
        3 Z                  z = fl(fl(g - C) * fl(1 / eps)): three roundings, and LSE is non-expansive in z
        2 Z                  z - m, |z - m| <= 2 Z
        n + 2 EXP_ULP        the sum's relative error: each exp within EXP_ULP ulp (an ulp is at most 2 u of the value), at
                             most n - 1 additions of positive terms in any order; log moves by as much
        2 LOG_ULP log n      log(s), 1 <= s <= n
        Z + log n            m + log(s)
        2 LOG_ULP log n      the constant log(n)
        Z + 2 log n          the subtraction of it
    and, not scaled by eps, u F for the final product (F = max |f|, |g| over all steps):
        d_step = eps u (7 Z + n + 2 EXP_ULP + (4 LOG_ULP + 3) log n) + u F.
  * ot = sum f / n_a + sum g / n_b moves by at most 2 e_K, and its two trees, two divisions and one addition lose at most
    (ceil(log2 n_a) + ceil(log2 n_b) + 4) u F.
  * err: x_j = (g_j - g'_j) / eps moves by at most dx = 2 e_K / eps + 3 u X (X = max |x_j| at that step), |expm1(x)| by
    at most exp(X + dx) dx, and expm1, the tree and the division lose (2 EXPM1_ULP + ceil(log2 n_b) + 2) u err.
  * mean_cost: the mean of the |dC_ij| plus (ceil(n_b / 64) + 6 + ceil(log2 n_a) + 2) u mean_cost for the lane chains, the
    butterfly, the tree and the division.
  * the divergence ot_ab - (ot_aa / 2 + ot_bb / 2): bound_ab + bound_aa / 2 + bound_bb / 2 + 2 u times the largest term.

EXP_ULP, LOG_ULP, EXPM1_ULP: the accuracy of the device's double-precision exp, log and expm1.  No table for the device
math library is at hand; 2 ulp each is a stated assumption (the HIP documentation is remembered to list 1 ulp for exp and
log).  They enter multiplied by eps u and are small beside the Z terms.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53                     # unit roundoff of fp64
EXP_ULP, LOG_ULP, EXPM1_ULP = 2, 2, 2

OK, NONFINITE, BAD_EPS, NOT_CONVERGED = 0, 1, 2, 4


def cost(a, b, p, dtype=LD):
    """C [n_a, n_b]: sum_e (a_ie - b_je)^2, its square root for p = 1"""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    c = np.stack([((row - b) ** 2).sum(axis=-1) for row in a])
    if p == 2:
        return c
    if p == 1:
        return np.sqrt(c)
    raise ValueError(p)


def _softmin(pot, C, eps, axis):
    """-eps (LSE over ``axis`` of (pot - C) / eps - log n), and the largest |z|"""
    z = ((pot[None, :] if axis == 1 else pot[:, None]) - C) / eps
    m = z.max(axis=axis, keepdims=True)
    s = np.exp(z - m).sum(axis=axis)
    n = C.dtype.type(C.shape[axis])
    return -eps * ((m.squeeze(axis) + np.log(s)) - np.log(n)), float(np.abs(z).max())


def iterate(C, eps, max_iter, tol=0.0, f_first=True):
    """The header's iteration on the cost matrix C in C's dtype.  ``f_first`` False starts with f = 0 and the column
    half-step instead (only the host tests use it).  Returns ot, err, iters, status, f, g, the err of every step run
    (``errs``) and what the bound needs: Z, F, X."""
    dt = C.dtype.type
    eps = dt(eps)
    if not f_first:
        r = iterate(np.ascontiguousarray(C.T), eps, max_iter, tol)
        r["f"], r["g"] = r["g"], r["f"]
        return r
    n_a, n_b = C.shape
    g = np.zeros(n_b, dtype=C.dtype)
    errs, Z, F, status = [], 0.0, 0.0, OK
    for k in range(1, max_iter + 1):
        f, z1 = _softmin(g, C, eps, 1)
        gn, z2 = _softmin(f, C, eps, 0)
        x = (g - gn) / eps
        errs.append(np.abs(np.expm1(x)).mean())
        g = gn
        Z, F = max(Z, z1, z2), max(F, float(np.abs(f).max()), float(np.abs(g).max()))
        X = float(np.abs(x).max())
        if tol > 0 and errs[-1] <= tol:
            break
    else:
        if tol > 0:
            status = NOT_CONVERGED
    return {"ot": f.mean() + g.mean(), "err": errs[-1], "iters": len(errs), "status": status, "f": f, "g": g, "errs": errs,
            "Z": Z, "F": F, "X": X}


def cost_bound(C, E, p):
    """[n_a, n_b]: the |dC_ij| of the module docstring (raised by 1e-9 of itself: C is the yardstick's, not the exact one)"""
    factor = (E + 1) if p == 2 else (E + 1) / 2 + 1
    return np.asarray(C, dtype=np.float64) * (factor * U * (1 + 1e-9))


def levels(n):
    return int(np.ceil(np.log2(n))) if n > 1 else 0


def mean_cost_bound(C, E, p):
    n_a, n_b = C.shape
    return float(cost_bound(C, E, p).mean() + (-(-n_b // 64) + 6 + levels(n_a) + 2) * U * float(C.mean()))


def forward_bound(C, eps, res, E, p):
    """{ot, err, f, g}: the bounds of the module docstring for the run ``res`` = iterate(C, eps, ..) of K = res["iters"] steps"""
    n_a, n_b = C.shape
    n, K, eps = max(n_a, n_b), res["iters"], float(eps)
    logn = float(np.log(n))
    d_step = eps * U * (7 * res["Z"] + n + 2 * EXP_ULP + (4 * LOG_ULP + 3) * logn) + U * res["F"]
    e_K = 2 * K * (float(cost_bound(C, E, p).max()) + d_step)
    dx = 2 * e_K / eps + 3 * U * res["X"]
    err = float(np.exp(res["X"] + dx)) * dx + (2 * EXPM1_ULP + levels(n_b) + 2) * U * float(res["err"])
    return {"ot": 2 * e_K + (levels(n_a) + levels(n_b) + 4) * U * res["F"], "err": err, "f": e_K, "g": e_K}


def divergence(ot_ab, ot_aa, ot_bb):
    return ot_ab - (ot_aa / 2 + ot_bb / 2)


def divergence_bound(b_ab, b_aa, b_bb, largest):
    return b_ab + b_aa / 2 + b_bb / 2 + 2 * U * float(largest)


def status(a, b, eps):
    """[P] int: the NONFINITE and BAD_EPS bits.  a, b [P, n, E] (or [n, E]: shared), eps [P]"""
    flags = [~np.isfinite(np.asarray(x).reshape((-1,) + np.asarray(x).shape[-2:])).all(axis=(1, 2)) for x in (a, b)]
    eps = np.asarray(eps, dtype=np.float64)
    return (flags[0] | flags[1]) * NONFINITE + (~(np.isfinite(eps) & (eps > 0))) * BAD_EPS


# ------------------------------------------------------------------------------------------------ test inputs
def sets(seed, P, n_a, n_b, E):
    """(a [P, n_a, E], b [P, n_b, E]) float32: seeded standard Gaussians, two independent draws"""
    rng = np.random.RandomState(seed)
    a, b = rng.standard_normal((P, n_a, E)), rng.standard_normal((P, n_b, E))
    return a.astype(np.float32), b.astype(np.float32)


def epsilon(a, b, p, rel_epsilon):
    """rel_epsilon x the mean self cost of the set a (of the cost between a and b where a is a single row, whose self
    cost is 0), rounded to float64: what a test hands to device and yardstick alike"""
    C = cost(a, a, p) if len(a) > 1 else cost(a, b, p)
    return float(np.float64(rel_epsilon) * np.float64(C.mean()))
