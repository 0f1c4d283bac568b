"""float64 yardstick of the device t-SNE (include/dt_hip_tsne.h): sklearn's method="exact" restated in plain numpy, so
that it needs no sklearn and keeps every quantity in float64 (sklearn takes the squared distances in float32).

  affinities(X, perplexity)            joint probabilities [n, n] from the centred float64 Gram matrix
  kl_grad(Y, P)                        KL(P || Q) and its gradient, as sklearn's _kl_divergence
  new_state(Y0) / descend(state, P, it_begin, it_end, params)
                                       sklearn's two _gradient_descent calls as one resumable loop

tests/test_tsne_host.py pins all three to sklearn.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
RUNNING, NO_PROGRESS, GRAD_NORM = 0, 1, 2


def default_params(n, **over):
    """sklearn's schedule for n rows (learning_rate "auto")"""
    p = dict(early_exaggeration=12.0, exaggeration_iters=250, learning_rate=None, momentum=(0.5, 0.8), min_gain=0.01,
             n_iter_check=50, n_iter_without_progress=(250, 300), min_grad_norm=1e-7)
    p.update(over)
    if p["learning_rate"] is None:
        p["learning_rate"] = max(n / p["early_exaggeration"] / 4.0, 50.0)
    return p


def walk_pair(seed, n, E):
    """a seeded random-walk teacher/student pair stacked to fp32 [n, E] rows (teacher rows first), with the common offset
    that trajectory states have"""
    rng = np.random.RandomState(seed)
    n_a = (n + 1) // 2
    a = np.cumsum(rng.standard_normal((n_a, E)), axis=0) + 5.0
    b = np.cumsum(0.8 * rng.standard_normal((n - n_a, E)), axis=0) + 5.0
    return np.vstack([a, b]).astype(np.float32)


def sq_distances(X):
    """D_ij = G_ii + G_jj - 2 G_ij of the centred float64 rows, clamped at 0, zero diagonal"""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    Xc = X - X.mean(axis=0)
    G = Xc @ Xc.T
    g = np.diag(G)
    D = np.maximum(g[:, None] + g[None, :] - 2.0 * G, 0.0)
    np.fill_diagonal(D, 0.0)
    return D


def conditional(D, perplexity):
    """sklearn's _binary_search_perplexity on float64 distances: rows of conditional probabilities, diagonal 0"""
    n = len(D)
    target = np.log(perplexity)
    C = np.zeros((n, n))
    for i in range(n):
        d = np.delete(D[i], i)
        beta, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(100):
            c = np.exp(-d * beta)
            s = c.sum()
            if s == 0.0:
                s = 1e-8
            c = c / s
            diff = np.log(s) + beta * np.dot(d, c) - target
            if abs(diff) <= 1e-5:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        C[i] = np.insert(c, i, 0.0)
    return C


def joint(C):
    P = C + C.T
    P = np.maximum(P / max(P.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P


def affinities(X, perplexity):
    return joint(conditional(sq_distances(X), perplexity))


def kl_grad(Y, P, alpha=1.0):
    """(KL(alpha P || Q), gradient [n, 2]) with w = 1 / (1 + |y_i - y_j|^2), Q = max(w / Z, eps)"""
    Y = np.asarray(Y, dtype=np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    W = 1.0 / (1.0 + (diff ** 2).sum(-1))
    np.fill_diagonal(W, 0.0)
    Q = np.maximum(W / W.sum(), EPS)
    aP = alpha * P
    off = ~np.eye(len(Y), dtype=bool)
    kl = float(np.sum(aP[off] * np.log(np.maximum(aP[off], EPS) / Q[off])))
    M = (aP - Q) * W
    np.fill_diagonal(M, 0.0)
    grad = 4.0 * (M[:, :, None] * diff).sum(axis=1)
    return kl, grad


def new_state(Y0):
    Y0 = np.array(Y0, dtype=np.float64)
    return dict(y=Y0, update=np.zeros_like(Y0), gains=np.ones_like(Y0), best_error=np.finfo(np.float64).max, best_iter=0,
                n_iter=0, stop=RUNNING)


def copy_state(s):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def descend(state, P, it_begin, it_end, params, trace=None):
    """Iterations [it_begin, it_end) on a copy of ``state``.  ``trace(it, state, grad)`` is called before each iteration's
    step, with the gradient of that iteration and the state it is applied to (after the stage reset)."""
    s = copy_state(state)
    exag = params["exaggeration_iters"]
    for it in range(it_begin, it_end):
        if s["stop"] != RUNNING:
            break
        if it == exag:
            s["update"][:] = 0.0
            s["gains"][:] = 1.0
            s["best_error"], s["best_iter"] = np.finfo(np.float64).max, it
        stage = 0 if it < exag else 1
        alpha = params["early_exaggeration"] if stage == 0 else 1.0
        error, grad = kl_grad(s["y"], P, alpha)
        if trace is not None:
            trace(it, s, grad)
        inc = s["update"] * grad < 0.0
        s["gains"] = np.maximum(np.where(inc, s["gains"] + 0.2, s["gains"] * 0.8), params["min_gain"])
        grad = grad * s["gains"]
        s["update"] = params["momentum"][stage] * s["update"] - params["learning_rate"] * grad
        s["y"] = s["y"] + s["update"]
        s["n_iter"] = it + 1
        if (it + 1) % params["n_iter_check"] == 0:
            if error < s["best_error"]:
                s["best_error"], s["best_iter"] = error, it
            elif it - s["best_iter"] > params["n_iter_without_progress"][stage]:
                s["stop"] = NO_PROGRESS
            if s["stop"] == RUNNING and np.sqrt((grad ** 2).sum()) <= params["min_grad_norm"]:
                s["stop"] = GRAD_NORM
    return s


def final_kl(state, P):
    return kl_grad(state["y"], P)[0]
