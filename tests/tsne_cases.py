"""The seeded problems that tests/test_tsne_host.py and tests/test_hip_tsne.py share, and the yardstick runs on them
(tests/tsne_ref64.py), each computed once per process and never changed afterwards.

A case is a random-walk pair of (n, E), its perplexity min(30, n // 5), the start Y0 = 1e-4 * N(0, 1) rounded to fp32,
the yardstick's affinities, its run from Y0 with the default schedule, and copies of the state before the iterations in
CAPTURE.

CHAOS_SPREAD[(n, E)] is s of DESIGN.md §9: the largest relative deviation of the yardstick's KL after 1000 iterations
under 8 relative perturbations of Y0 of size 1e-15 (Y0 * (1 + 1e-15 * RandomState(1000 + k).standard_normal(shape)),
k = 0 .. 7), measured on the CPU for these seeds: 8.005e-4 at (102, 768) and 7.282e-3 at (130, 48), rounded up.  A KL
may exceed the yardstick's by 3 s: the factor covers the tail that 8 draws undersample.
"""
import functools

import numpy as np

import tsne_ref64 as ref

SEEDS = {(12, 12): 3, (102, 768): 5, (130, 48): 7, (65, 48): 11}
RUN_ITERS = {(12, 12): 0, (102, 768): 1000, (130, 48): 1000, (65, 48): 603}
CAPTURE = (0, 5, 249, 250, 300, 600)
CHAOS_SPREAD = {(102, 768): 8.1e-4, (130, 48): 7.3e-3}
CHAOS_FACTOR = 3.0


def rows(n, E):
    return ref.walk_pair(SEEDS[(n, E)], n, E)


def perplexity(n):
    return float(min(30, n // 5))


def start(n, E):
    return (1e-4 * np.random.RandomState(100 + SEEDS[(n, E)]).standard_normal((n, 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(n, E):
    """dict(X, perplexity, P, Y0, params, states {it: state before iteration it}, final, tie_margin): tie_margin is the
    smallest |update . grad| / (max|update| max|grad|) over the iterations it, it+1, it+2 of every captured it except the
    first iteration of a stage (where update is zero and the product is exactly 0)"""
    X = rows(n, E)
    P = ref.affinities(X, perplexity(n))
    Y0 = start(n, E)
    params = ref.default_params(n)
    tested = {c + d for c in CAPTURE for d in range(3)} - {0, params["exaggeration_iters"]}
    states, margin = {}, [np.inf]

    def watch(it, s, grad):
        if it in tested:
            margin[0] = min(margin[0], np.abs(s["update"] * grad).min() / (np.abs(s["update"]).max() * np.abs(grad).max()))

    s = ref.new_state(Y0)
    for it in range(RUN_ITERS[(n, E)]):      # one iteration at a time: the state before `it` precedes its stage reset
        if it in CAPTURE:
            states[it] = ref.copy_state(s)
        s = ref.descend(s, P, it, it + 1, params, trace=watch)
    P.setflags(write=False)
    return dict(X=X, perplexity=perplexity(n), P=P, Y0=Y0, params=params, states=states, final=s, tie_margin=margin[0])



def tie_margin(state, P, it_begin, it_end, params):
    """the smallest |update . grad| / (max|update| max|grad|) of the yardstick's iterations [it_begin, it_end) from state"""
    worst = [np.inf]

    def watch(it, s, grad):
        worst[0] = min(worst[0], np.abs(s["update"] * grad).min() / (np.abs(s["update"]).max() * np.abs(grad).max()))
    ref.descend(state, P, it_begin, it_end, params, trace=watch)
    return worst[0]
