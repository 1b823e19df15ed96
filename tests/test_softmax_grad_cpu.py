"""The NumPy mirror of gpmi_softmax_grad (tests/softmax_grad_ref.py) against central differences of softmax_ref.fit's own
log q, against the dense (K_blk^-1 + W)^-1, and -- at C = 2, where the softmax model with kernel K is the binary model
with kernel 2 K -- against the binary classifier's mirror, which is held to scikit-learn; the declarations of the new
entry point; the tuner's loop on a context served by the mirror; and the table of rounding figures that
tests/test_softmax_grad_gpu.py takes its bars from.

THE BARS.  As in tests/test_laplace_grad_cpu.py: rounding_figure(case) is the largest change of the mirror's gradient,
relative to its largest |component|, over five seeds when every element of K is multiplied symmetrically by
1 + 2^-52 u, u uniform in [-1, 1].  ROUNDING holds the figure of every case, measured once with
`python tests/test_softmax_grad_cpu.py`; the GPU bar of a case is 50 x its figure, floored at 1e-11.
test_rounding_table_is_current re-measures the cases up to N = 300 and holds the table within a factor 5."""
import os
import re

import numpy as np
import pytest
from scipy.linalg import block_diag

import laplace_grad_ref as LG
import softmax_grad_ref as G
import softmax_ref as S
from conftest import GOLDEN, ROOT

FIT_TOL = 1e-13
CD_BAR = 1e-8              # central differences, h = 1e-5: 50 x the 2.1e-10 measured on blobs(40, 2, 3, 1)

ELL = {1: 1.0, 3: 1.5, 8: 3.0, 16: 4.0, 33: 6.0}
# (N, d, C): under one tile, the tile edge and one past it, several tiles; every width of the trace kernel and, d = 33,
# its multi-launch path; C <= 4 one pass of the multi-vector product, C = 5 two, C = 10 three
SHAPES = [(50, 1, 2), (50, 3, 3), (128, 8, 3), (129, 3, 4), (129, 16, 5), (129, 33, 3), (300, 8, 10), (300, 1, 3),
          (1024, 3, 3)]
# id -> (N, d, C, sigma, l, ard)
CASES = {}
for _N, _d, _C in SHAPES:
    for _ard in (False, True):
        CASES["N%d_d%d_C%d_%s" % (_N, _d, _C, "ard" if _ard else "iso")] = (_N, _d, _C, 1.5, ELL[_d], _ard)


def make_case(name):
    """-> (X, labels, C, sigma, l, r or None); r as make_case of tests/test_laplace_grad_cpu.py"""
    N, d, C, sigma, l, ard = CASES[name]
    X, lab, _ = S.blobs(N, d, C, N + d + C)
    r = 0.6 + 1.2 * np.random.default_rng(1000 + d).random(d) if ard else None
    return X, lab, C, sigma, l, r


def n2000_case():
    """the one case above N = 1024: the inputs of tests/golden/laplace/moons_N2000_d2, its two labels as classes 0 / 1
    and the points of class 1 left of x_0 = 0 as a third class"""
    g = np.load(os.path.join(GOLDEN, "laplace", "moons_N2000_d2.npz"))
    X = g["X"]
    lab = np.where(g["y"] > 0, 1, 0)
    lab[(lab == 1) & (X[:, 0] < 0)] = 2
    return X, lab, 3, float(g["sigma"]), float(g["l"]), np.array([0.8, 1.5])


def c2_case():
    """C = 2: (X, labels, y in {-1, +1}, sigma, l, r); label 0 is y = +1 (f_0 - f_1 is the binary latent function)"""
    X, lab, _ = S.blobs(129, 3, 2, 5)
    return X, lab, np.where(lab == 0, 1.0, -1.0), 1.7, 1.3, 1.0 + 0.3 * np.arange(3)


def sym_noise(N, seed):
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, (N, N))
    return np.tril(u) + np.tril(u, -1).T


def rounding_figure(X, lab, C, sigma, l, r, seeds=5):
    base = G.flat(G.log_q_and_gradient(X, lab, C, sigma, l, r, tol=FIT_TOL))
    worst = 0.0
    for seed in range(seeds):
        g = G.flat(G.log_q_and_gradient(X, lab, C, sigma, l, r, tol=FIT_TOL, perturb=2.0 ** -52 * sym_noise(X.shape[0], seed)))
        worst = max(worst, float(np.max(np.abs(g - base)) / np.max(np.abs(base))))
    return worst


def binary_rounding_figure(X, y, sigma, l, r, seeds=5):
    base = LG.flat(LG.log_q_and_gradient(X, y, sigma, l, r, tol=FIT_TOL))
    worst = 0.0
    for seed in range(seeds):
        g = LG.flat(LG.log_q_and_gradient(X, y, sigma, l, r, tol=FIT_TOL, perturb=2.0 ** -52 * sym_noise(X.shape[0], seed)))
        worst = max(worst, float(np.max(np.abs(g - base)) / np.max(np.abs(base))))
    return worst


# measured by this module's main(); see the module docstring
ROUNDING = {
    "N50_d1_C2_iso": 4.4e-14,
    "N50_d1_C2_ard": 5.6e-14,
    "N50_d3_C3_iso": 1.5e-15,
    "N50_d3_C3_ard": 3e-15,
    "N128_d8_C3_iso": 1.6e-14,
    "N128_d8_C3_ard": 5.6e-15,
    "N129_d3_C4_iso": 1.3e-14,
    "N129_d3_C4_ard": 7.1e-15,
    "N129_d16_C5_iso": 3.7e-15,
    "N129_d16_C5_ard": 8.2e-15,
    "N129_d33_C3_iso": 4.8e-15,
    "N129_d33_C3_ard": 8.7e-15,
    "N300_d8_C10_iso": 6.1e-15,
    "N300_d8_C10_ard": 5e-15,
    "N300_d1_C3_iso": 9.6e-13,
    "N300_d1_C3_ard": 1.8e-12,
    "N1024_d3_C3_iso": 3.6e-13,
    "N1024_d3_C3_ard": 6.7e-14,
    "moons_N2000_d2_C3_ard": 3.1e-09,
    "c2_softmax": 9.5e-15,
    "c2_binary": 3.6e-16,
}


def gpu_bar(figure):
    return max(50.0 * figure, 1e-11)


def central_differences(X, lab, C, sigma, l, r, h=1e-5):
    d = X.shape[1]
    fd = np.empty(d + 2)
    for k in range(d + 2):
        def log_q(e):
            rr, ll, ss = r.copy(), l, sigma
            if k < d:
                rr[k] += e
            elif k == d:
                ll += e
            else:
                ss += e
            return S.fit(X / rr, lab, C, ss, ll, tol=FIT_TOL)["log_q"]
        fd[k] = (log_q(h) - log_q(-h)) / (2 * h)
    return fd


# the issue's three problems (ARD r = 1 + 0.3 k, sigma = 1.7, l = 1.3) and one with d = 8, C = 5
CD_PROBLEMS = {"blobs_40_2_3_1": (40, 2, 3, 1), "blobs_60_3_4_2": (60, 3, 4, 2), "blobs_30_1_2_3": (30, 1, 2, 3),
               "blobs_48_8_5_4": (48, 8, 5, 4)}
_cd_cache = {}


def cd_problem(name):
    """-> (X, labels, C, sigma, l, r, central differences): computed once, shared by the three tests below"""
    if name not in _cd_cache:
        N, d, C, seed = CD_PROBLEMS[name]
        X, lab, _ = S.blobs(N, d, C, seed)
        r = 1.0 + 0.3 * np.arange(d)
        sigma, l = (1.7, 1.3) if d < 8 else (1.7, 3.0)
        _cd_cache[name] = (X, lab, C, sigma, l, r, central_differences(X, lab, C, sigma, l, r))
    return _cd_cache[name]


def cd_miss(name, **controls):
    X, lab, C, sigma, l, r, fd = cd_problem(name)
    res = G.log_q_and_gradient(X, lab, C, sigma, l, r, tol=FIT_TOL, **controls)
    assert res["fit"]["converged"]
    g = G.flat(res)
    return float(np.max(np.abs(fd - g)) / np.max(np.abs(fd)))


@pytest.mark.parametrize("name", list(CD_PROBLEMS))
def test_mirror_matches_central_differences(name):
    err = cd_miss(name)
    print("%s: mirror - central differences %.3g" % (name, err))
    assert err <= CD_BAR


@pytest.mark.parametrize("name", list(CD_PROBLEMS))
def test_flipped_s2_is_caught(name):
    """the gradient with -s2 misses the same differences by 1.14, 0.98, 0.87 and 1.4 of the largest component on the four
    problems (measured); at least 1000 x the bar is asked"""
    miss = cd_miss(name, flip_s2=True)
    print("%s: with -s2 the miss is %.3g" % (name, miss))
    assert miss >= 1000 * CD_BAR


@pytest.mark.parametrize("name", list(CD_PROBLEMS))
def test_dropped_gamma_is_caught(name):
    """without Gamma the miss is 1.15, 0.69, 1.04 and 0.79 of the largest component on the four problems (measured)"""
    miss = cd_miss(name, drop_gamma=True)
    print("%s: without Gamma the miss is %.3g" % (name, miss))
    assert miss >= 1000 * CD_BAR


@pytest.mark.parametrize("name", ["blobs_40_2_3_1", "blobs_30_1_2_3"])
def test_point_covariances_match_the_dense_posterior(name):
    """Sigma_i against the i-th C x C block of the dense (K_blk^-1 + W)^-1, formed as K_blk (I + W K_blk)^-1 (W is
    singular, so nothing is inverted but I + W K_blk); then the closed form of s2 against the explicit contraction"""
    X, lab, C, sigma, l, r, _ = cd_problem(name)
    fit = S.fit(X / r, lab, C, sigma, l, tol=FIT_TOL)
    N = X.shape[0]
    P, K = fit["P"], fit["K"]
    Kb = block_diag(*[K] * C)
    Pi = np.vstack([np.diag(P[c]) for c in range(C)])            # Cn x n
    W = np.diag(P.reshape(-1)) - Pi @ Pi.T
    dense = Kb @ np.linalg.inv(np.eye(C * N) + W @ Kb)
    Sig = G.point_covariances(fit, sigma * sigma)
    idx = np.arange(C) * N
    worst = max(float(np.max(np.abs(Sig[i] - dense[np.ix_(idx + i, idx + i)]))) for i in range(N))
    print("%s: Sigma_i - dense %.3g" % (name, worst))
    assert worst <= 1e-12
    # the closed form of s2 against the explicit contraction with dW_i[p, q]/df_c
    s2 = G.third_derivative_term(Sig, P)
    for i in (0, N // 2, N - 1):
        p = P[:, i]
        for c in range(C):
            dp = p[c] * ((np.arange(C) == c) - p)                # dpi/df_c
            dW = np.diag(dp) - np.outer(dp, p) - np.outer(p, dp)
            assert abs(s2[c, i] + 0.5 * np.sum(Sig[i] * dW)) <= 1e-14


def test_two_classes_are_the_binary_model_with_twice_the_kernel():
    X, lab, y, sigma, l, r = c2_case()
    a = G.log_q_and_gradient(X, lab, 2, sigma, l, r, tol=FIT_TOL)
    b = LG.log_q_and_gradient(X, y, np.sqrt(2.0) * sigma, l, r, tol=FIT_TOL)
    fb = LG.flat(b)
    fb[-1] *= np.sqrt(2.0)
    err = float(np.max(np.abs(G.flat(a) - fb)) / np.max(np.abs(fb)))
    print("C = 2: softmax - binary %.3g, log q %.3g apart" % (err, abs(a["log_q"] - b["log_q"]) / abs(b["log_q"])))
    assert abs(a["log_q"] - b["log_q"]) <= 1e-12 * abs(b["log_q"])
    assert err <= 1e-12


def test_isotropic_and_relative_conventions():
    X, lab, C, sigma, l, r = make_case("N129_d3_C4_ard")
    a = G.log_q_and_gradient(X, lab, C, sigma, l, r, tol=FIT_TOL)
    assert abs(l * a["d_l"] - np.sum(r * a["d_r"])) <= 1e-12 * abs(l * a["d_l"])
    b = G.log_q_and_gradient(X, lab, C, sigma, 1.0, l * r, tol=FIT_TOL)
    assert abs(a["log_q"] - b["log_q"]) <= 1e-12 * abs(a["log_q"])
    assert np.max(np.abs(b["d_r"] * l - a["d_r"])) <= 1e-10 * np.max(np.abs(a["d_r"]))


def test_header_and_signatures_declare_the_entry_point():
    import ctypes as C

    from gaussian_process_amd import _lib
    text = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    assert re.search(r"int gpmi_softmax_grad\(gpmi_ctx\* ctx, double\* d_r, double\* d_ell, double\* d_sigma\);", text)
    assert re.search(r"#define GPMI_ABI_VERSION 4\b", text) and re.search(r"GPMI_T_COUNT = 16\b", text)
    dp = C.POINTER(C.c_double)
    assert _lib.SIGNATURES["gpmi_softmax_grad"] == [C.c_void_p, dp, dp, dp]
    assert _lib.ABI_VERSION == 4 and _lib.T_COUNT == 16


def test_rounding_table_covers_every_case():
    assert sorted(ROUNDING) == sorted(list(CASES) + ["moons_N2000_d2_C3_ard", "c2_softmax", "c2_binary"])
    # the moons case is the ill-conditioned one (3.1e-9; every other figure is below 2e-12)
    assert all(0.0 < v < 1e-8 for v in ROUNDING.values())


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[0] <= 300])
def test_rounding_table_is_current(name):
    fig = rounding_figure(*make_case(name))
    print("%s: rounding figure %.3g (table %.3g)" % (name, fig, ROUNDING[name]))
    assert ROUNDING[name] / 5 <= fig <= 5 * ROUNDING[name]


# ---- the tuner's loop on a context that serves the mirror ---------------------------------------------------------------
def test_tuner_never_decreases_on_the_mirror():
    import warnings

    from gaussian_process_amd import GP_multi_classification as M
    X, lab, _ = S.blobs(60, 2, 3, 11)
    c = G.MirrorContext()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ls, sigma, log_q, trace = M.tune_hyperparms_classification(X, lab, sigma=1.0, lengthscales=5.0, ctx=c, max_iter=12)
    assert ls.shape == (2,) and sigma > 0 and len(trace) >= 2
    assert np.all(np.diff(trace) >= 0) and trace[-1] > trace[0] and log_q == trace[-1]
    # the fit left in the context is the returned point's
    assert np.allclose(c.r, ls, rtol=0, atol=0) and c.res["log_q"] == log_q and c.n_classes == 3
    d_r, _, d_sigma = c.softmax_grad()
    gnorm = np.linalg.norm(np.concatenate([d_r * ls, [d_sigma * sigma]]))
    assert gnorm <= 1e-6 or (len(trace) - 1 == 12 and any(issubclass(x.category, RuntimeWarning) for x in w))


def test_log_q_and_gradient_conventions_on_the_mirror():
    from gaussian_process_amd import GP_multi_classification as M
    X, lab, _ = S.blobs(60, 3, 3, 5)
    c = G.MirrorContext()
    ls = np.array([1.2, 2.0, 0.8])
    log_q, d_ls, d_sigma = M.log_q_and_gradient(X, lab, 1.5, ls, ctx=c)
    ref = G.log_q_and_gradient(X, lab, 3, 1.5, 1.0, ls, tol=FIT_TOL)
    assert log_q == ref["log_q"] and np.array_equal(d_ls, ref["d_r"]) and d_sigma == ref["d_sigma"]
    log_q, d_l, d_sigma = M.log_q_and_gradient(X, lab, 1.5, 2.0, n_classes=3, ctx=c)
    ref = G.log_q_and_gradient(X, lab, 3, 1.5, 2.0, None, tol=FIT_TOL)
    assert np.ndim(d_l) == 0 and d_l == ref["d_l"] and d_sigma == ref["d_sigma"] and c.r is None


def test_tuner_refuses_bad_start():
    from gaussian_process_amd import GP_multi_classification as M
    c = G.MirrorContext()
    lab = np.array([0, 1, 2, 0, 1])
    with pytest.raises(ValueError):
        M.tune_hyperparms_classification(np.zeros((5, 2)), lab, lengthscales=[1.0, -1.0], ctx=c)
    with pytest.raises(ValueError):
        M.tune_hyperparms_classification(np.zeros((5, 2)), lab, lengthscales=[1.0, 2.0, 3.0], ctx=c)
    with pytest.raises(ValueError):
        M.tune_hyperparms_classification(np.zeros((5, 2)), lab, sigma=0.0, ctx=c)
    with pytest.raises(ValueError):
        M.tune_hyperparms_classification(np.zeros((5, 2)), lab, n_classes=2, ctx=c)
    assert c.fits == 0


def main():
    print("ROUNDING = {")
    for name in CASES:
        print('    "%s": %.2g,' % (name, rounding_figure(*make_case(name))), flush=True)
    print('    "moons_N2000_d2_C3_ard": %.2g,' % rounding_figure(*n2000_case()), flush=True)
    X, lab, y, sigma, l, r = c2_case()
    print('    "c2_softmax": %.2g,' % rounding_figure(X, lab, 2, sigma, l, r), flush=True)
    print('    "c2_binary": %.2g,' % binary_rounding_figure(X, y, np.sqrt(2.0) * sigma, l, r), flush=True)
    print("}")


if __name__ == "__main__":
    main()
