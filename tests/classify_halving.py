"""The step-halving problems of the classification tests -- TEST INFRASTRUCTURE shared by
tests/test_classify_halving_cpu.py (the preconditions, on the mirrors alone) and tests/test_classify_halving_gpu.py
(the GPU against the mirrors): the problems, the mirror runs (each computed once per process) and the mirrors' own
sensitivity to one rounding of K, which sets the bounds of the GPU comparison.

binary    problem(257, 2, seed=257) of tests/test_laplace_gpu.py with sigma = 300, l = 0.3 (cond(K) about 3.8e6).  The
          Newton iteration overshoots after steps 10 and 11 and halves twice each time; the full run converges in 18
          steps.
softmax2  the same data as a softmax problem with C = 2 and sigma = 300 / sqrt(2): the same iteration (C = 2 is the
          binary classifier with kernel 2 K) through the other mirror and the other device path.
softmax3  blobs(200, 2, 3, seed=0) of tests/softmax_ref.py with sigma = 300, l = 0.3 (cond(K) about 1.4e7): two
          halvings after step 6, converged in 17 steps.  Found by a search over seeds 0..5, N in {129, 200},
          sigma in {30, 100, 300} and l in {0.15, 0.3, 0.6} with d = 2; only sigma = 300 halved."""
import functools

import numpy as np

import laplace_ref as LR
import softmax_ref as SR

KINDS = ("binary", "softmax2", "softmax3")
RUNS = ("capped", "full")
QUANTITIES = ("F", "log_q", "mean", "cov", "prob")
NOISE_SEEDS = (0, 1, 2, 3, 4)
DRAWS = 200
ELL = 0.3
SIGMA = {"binary": 300.0, "softmax2": 300.0 / np.sqrt(2), "softmax3": 300.0}
CLASSES = {"binary": None, "softmax2": 2, "softmax3": 3}
FIRST_HALVING = {"binary": 10, "softmax2": 10, "softmax3": 6}    # the Newton step after which the first halving comes
CAP = {k: v + 2 for k, v in FIRST_HALVING.items()}               # max_iter of the capped run: two steps past it

try:
    from threadpoolctl import threadpool_limits       # these matrices are small: one BLAS thread is the fastest
except ImportError:
    import contextlib

    def threadpool_limits(limits=None):
        return contextlib.nullcontext()


@functools.lru_cache(maxsize=None)
def data(kind):
    """-> X, labels (+-1 for binary, 0 .. C-1 for softmax), X_test"""
    if kind == "softmax3":
        return SR.blobs(200, 2, 3, 0)
    rng = np.random.default_rng(257)                   # problem(257, 2, 257) of tests/test_laplace_gpu.py
    y = np.where(rng.random(257 + 300) < 0.5, -1.0, 1.0)
    X = rng.standard_normal((257 + 300, 2)) * 1.5 + y[:, None] * (1.0 / np.sqrt(2))
    if kind == "softmax2":
        y = np.where(y > 0, 0, 1)                      # label 0 <-> y = +1
    return X[:257], y[:257], X[257:]


def normals(kind):
    return np.random.default_rng(257).standard_normal((DRAWS, CLASSES[kind]))


def max_iter_of(kind, run):
    return CAP[kind] if run == "capped" else 100


@functools.lru_cache(maxsize=None)
def kernel(kind):
    K = LR.rbf(data(kind)[0], data(kind)[0], SIGMA[kind], ELL)
    K.setflags(write=False)
    return K


def mirror(kind, run, K=None, max_halvings=20):
    """-> dict(F, log_q, mean, cov, prob, iters, converged, halvings, decisions); K defaults to the exact kernel"""
    X, y, Xs = data(kind)
    sg = SIGMA[kind]
    K = kernel(kind) if K is None else K
    with threadpool_limits(limits=1):
        if kind == "binary":
            ft = LR.laplace_fit(X, y, sg, ELL, max_iter=max_iter_of(kind, run), K=K, max_halvings=max_halvings)
            mean, cov, prob, _ = LR.laplace_predict(ft, X, Xs, sg, ELL)
            F = ft["f"]
        else:
            ft = SR.fit(X, y, CLASSES[kind], sg, ELL, max_iter=max_iter_of(kind, run), K=K, max_halvings=max_halvings)
            mean, cov = SR.predict(ft, X, Xs, sg, ELL)
            prob = SR.proba(mean, cov, normals(kind))
            F = ft["F"]
    return dict(F=F, log_q=ft["log_q"], mean=mean, cov=cov, prob=prob, iters=ft["iters"], converged=ft["converged"],
                halvings=ft["halvings"], decisions=ft["decisions"])


@functools.lru_cache(maxsize=None)
def reference(kind, run):
    return mirror(kind, run)


@functools.lru_cache(maxsize=None)
def without_halving(kind, run):
    return mirror(kind, run, max_halvings=0)


def gaps(kind, a, b):
    """the five figures of the GPU tests, a against the reference b: F, mean relative to the reference's largest entry,
    log q relative, cov relative to sigma^2, prob absolute"""
    return dict(F=np.max(np.abs(a["F"] - b["F"])) / np.max(np.abs(b["F"])),
                log_q=abs(a["log_q"] - b["log_q"]) / abs(b["log_q"]),
                mean=np.max(np.abs(a["mean"] - b["mean"])) / np.max(np.abs(b["mean"])),
                cov=np.max(np.abs(a["cov"] - b["cov"])) / SIGMA[kind] ** 2,
                prob=np.max(np.abs(a["prob"] - b["prob"])))


@functools.lru_cache(maxsize=None)
def sensitivity(kind, run):
    """The largest movement of each figure of gaps() when every entry of K is multiplied by 1 + 2^-53 g, g standard
    normal and symmetric, over NOISE_SEEDS: what one rounding of the kernel matrix does to the mirror itself."""
    ref = reference(kind, run)
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for seed in NOISE_SEEDS:
        N = kernel(kind).shape[0]
        g = np.tril(np.random.default_rng(1000 + seed).standard_normal((N, N)))
        g = g + np.tril(g, -1).T
        moved = gaps(kind, mirror(kind, run, K=kernel(kind) * (1.0 + 2.0 ** -53 * g)), ref)
        for q in QUANTITIES:
            worst[q] = max(worst[q], moved[q])
    return worst
