"""The cases on which gpmi_predict_grad_resident is held to the mirror (tests/predgrad_ref.py), with their references and
bars, computed once per process and shared between tests/test_predgrad_cpu.py (which prints the table) and
tests/test_predgrad_gpu.py (which holds the device to it).

The bar of a case: 20 x what the float64 mirror misses of the long-double mirror in the normalisation |got - ref| / S,
and never below 1e-13 -- the device sums in another order and with its own exp; a factor of 20 over float64's own
distance is the margin the other route modules use.  It never comes from a device run.

Test infrastructure."""
import numpy as np

import predgrad_ref as G

FLOOR, MARGIN = 1e-13, 20.0
SIGMA = 1.3

# name: (N, d, n, kind, lengthscales, noise).  N = 641 is six blocks with a partial last one; n covers one point, a partial
# row group, exactly one, one more, several, and more than a 128-row tile; d the four widths of the pass (4, 8, 32) and 1.
CASES = {
    "rbf_d3_n37_ard_1e-4": (641, 3, 37, "rbf", True, 1e-4),
    "rbf_d3_n17_iso_0.1": (641, 3, 17, "rbf", False, 0.1),
    "rbf_d1_n1_ard": (641, 1, 1, "rbf", True, 1e-3),
    "rbf_d8_n200_iso": (641, 8, 200, "rbf", False, 1e-3),
    "rbf_d32_n17_ard": (641, 32, 17, "rbf", True, 1e-2),
    "m12_d1_n5_iso": (641, 1, 5, "matern12", False, 1e-2),
    "m12_d3_n16_ard": (641, 3, 16, "matern12", True, 1e-2),
    "m32_d8_n16_ard": (641, 8, 16, "matern32", True, 1e-3),
    "m32_d1_n37_iso": (641, 1, 37, "matern32", False, 1e-3),
    "m52_d32_n200_iso": (641, 32, 200, "matern52", False, 1e-2),
    "m52_d3_n5_ard": (641, 3, 5, "matern52", True, 1e-3),
    "rbf_d8_n16_ard_N1500": (1500, 8, 16, "rbf", True, 1e-3),
}


def ell(d):
    """a lengthscale that keeps neighbours correlated in [-2, 2]^d"""
    return 0.8 * np.sqrt(d)


_cache = {}


def case(name):
    """-> dict: X, y, Xs, r, kind, sigma, l, noise, ld (the long-double mirror), f64 (the float64 mirror), miss_mu / miss_var
    (float64 against long double) and bar_mu / bar_var"""
    if name not in _cache:
        N, d, n, kind, ard, noise = CASES[name]
        X, y, Xs, r = G.problem(N, d, n, seed=1000 + len(name) + N + d + n, lengthscales=ard)
        l = ell(d)
        ref = G.predict_grad(G.fit(X, y, r, kind, SIGMA, l, noise, np.longdouble), Xs)
        f64 = G.predict_grad(G.fit(X, y, r, kind, SIGMA, l, noise, np.float64), Xs)
        miss_mu = G.err(f64["dmu"], ref["dmu"], ref["S_mu"])
        miss_var = G.err(f64["dvar"], ref["dvar"], ref["S_var"])
        c = dict(X=X, y=y, Xs=Xs, r=r, kind=kind, sigma=SIGMA, l=l, noise=noise, ld=ref, f64=f64, miss_mu=miss_mu,
                 miss_var=miss_var, bar_mu=max(MARGIN * miss_mu, FLOOR), bar_var=max(MARGIN * miss_var, FLOOR))
        for v in (X, y, Xs):
            v.setflags(write=False)
        _cache[name] = c
    return _cache[name]
