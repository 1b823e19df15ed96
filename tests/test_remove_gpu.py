"""GPContext.remove (gpmi_remove) against a fresh fit of the surviving points in a second context: the factor at the
componentwise bar of the panel kernels (tests/panel_ref.py: |K_y - L L^T| <= 2 n u |L| |L^T|), the LML, m, alpha, diag(L),
predictions, ARD and leave-one-out gradients at the bars of tests/test_append_gpu.py, and the leading J0 x J0 block bit
for bit.  Single calls cover the smallest fit, one block, the y row moving, the front, middle and end of a fit, a block
edge, two and ten sweeps, a nine-launch chain, 16- and 128-tile edges and a sampled 2300; the pairs up to 300 points also
run at d = 1, with a Matern kernel, with ARD lengthscales and on a first-generation factor; one fit is the composite
kernel's.  Then ownership (a backward solve first), determinism, the stored inverses (predict, both append routes, append
and remove again), sequences (130 single removals; 130 sliding-window steps), the refusals and the resident state.

Noise is 1e-2.  Every case prints its figures.  Above 700 points the factor's ratio is taken on a sample of the rows
from J0 on (_factor_ratio).  Sequences are held by m, diag, alpha, the LML and the predictions; their ratio is printed
(tests/test_remove_cpu.py says why)."""
import ctypes as C

import numpy as np
import pytest

import ard_ref
import matern_ref
import panel_ref as R

pytestmark = pytest.mark.gpu

LML_RTOL, M_RTOL, ALPHA_RTOL, DIAG_RTOL = 1e-10, 1e-9, 1e-8, 1e-11      # tests/test_append_gpu.py
MU_ATOL, SD_ATOL = 1e-9, 1e-9
GRAD_RTOL = 1e-8
SIGMA, ELL, NOISE = 1.2, 1.5, 1e-2
R_ARD = np.array([0.7, 1.0, 1.6, 0.9, 2.5, 1.2, 0.8, 1.1])

EDGES = [15, 16, 127, 128, 129, 255, 256, 511, 512, 1023, 1024, 1025, 767, 768, 1087, 1088]
SINGLE = [(2, [0]), (128, [5]), (129, [128]), (129, [0]), (200, [0]), (200, [100]), (200, [199]), (256, [127, 128]),
          (300, [i * 300 // 17 for i in range(17)]), (300, list(range(0, 300, 2))),
          (1100, [0]), (1100, [1099]), (1100, EDGES), (2300, [7, 1000, 1001, 1666, 2299])]
SMALL = [(N, idx) for N, idx in SINGLE if N <= 300]
# (N, idx, d, kernel, ard, fused)
CASES = ([(N, idx, 8, "rbf", False, 1) for N, idx in SINGLE] +
         [(N, idx, d, kern, ard, fused) for N, idx in SMALL
          for d, kern, ard, fused in ((1, "rbf", False, 1), (8, "matern52", False, 1), (8, "rbf", True, 1), (8, "rbf", False, 0))])


def _id(case):
    N, idx, d, kern, ard, fused = case
    return "N%d-k%d-from%d-d%d-%s%s%s" % (N, len(idx), min(idx), d, kern, "-ard" if ard else "", "" if fused else "-gen1")


@pytest.fixture(scope="module")
def actx():
    """the context that removes; options, kernel and lengthscales are context state, so it is this module's own"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fctx():
    """the context of the fresh fits"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


def relmax(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


_data = {}


def _problem(N, d):
    if (N, d) not in _data:
        X, y = ard_ref.problem(N, d, seed=3000 + N + d)
        rng = np.random.default_rng(N + d)
        Xs = rng.uniform(0.0, 4.0, size=(40, d))
        for a in (X, y, Xs):
            a.setflags(write=False)
        _data[N, d] = (X, y, Xs)
    return _data[N, d]


def _survivors(N, idx):
    return np.setdiff1d(np.arange(N), np.asarray(idx))


def _ratio_rows(S, G, rows):
    """panel_ref.potrf_ratio on the given rows only (rows are independent in it)"""
    n = S.shape[0]
    L = np.tril(G)
    Ll, La = L.astype(R.LD), np.abs(L)
    rows = np.asarray(rows)
    worst = 0.0
    for c0 in range(0, int(rows.max()) + 1, 128):
        c1 = min(n, c0 + 128)
        sel = rows[rows >= c0]
        Rr = np.abs(S[sel, c0:c1].astype(R.LD) - Ll[sel, :c1] @ Ll[c0:c1, :c1].T)
        D = (La[sel, :c1] @ La[c0:c1, :c1].T).astype(R.LD) * (n * R.U)
        low = sel[:, None] >= np.arange(c0, c1)[None, :]
        worst = max(worst, R._ratio(Rr[low], D[low]))
    return worst


def _factor_ratio(S, G, J0):
    """panel_ref.potrf_ratio on the whole factor up to 700 points; beyond, on a sample of the rows from J0 on (the rows
    below are the resident ones bit for bit, which every case asserts): the first, the last and a seeded sample, 64 rows
    in all -- the long-double residual runs without BLAS and a case is allowed a few seconds.  m, diag(L) and alpha
    against the fresh fit cover every row."""
    n = S.shape[0]
    if n <= 700:
        return R.potrf_ratio(S, G)
    rows = np.arange(min(J0, n - 1), n)
    if rows.size > 64:
        rng = np.random.default_rng(n)
        keep = {int(rows[0]), int(rows[-1])}
        keep |= set(int(v) for v in rng.choice(rows, 64 - len(keep), replace=False))
        rows = np.array(sorted(keep))
    return _ratio_rows(S, G, rows)


def _configure(c, kern, fused=1, reserve=0, route=-1, spare=0):
    c.set_kernel(kern)
    c.set_option("panel_fused", fused)
    c.set_option("reserve", reserve)
    c.set_option("append_skinny", route)
    c.set_option("remove_keep_spare", spare)


def _kernel_matrix(c, kern, X, ard):
    Z = X / R_ARD[:X.shape[1]] if ard else X
    K = c.rbf(Z, Z, SIGMA, ELL) if kern == "rbf" else c.cov(kern, Z, Z, SIGMA, ELL)
    K[np.diag_indices_from(K)] += NOISE
    return K


_refs = {}


def _scales(key, X, y, d, kern, ard):
    """the cancellation scales of the gradients from the dense mirror, once per surviving set"""
    if key not in _refs:
        r = R_ARD[:d] if ard else np.ones(d)
        if kern == "rbf":
            _refs[key] = ard_ref.lml_and_grad(X, y, r, SIGMA, ELL, NOISE)
        else:
            _refs[key] = matern_ref.lml_and_grad(X, y, r, 2.5, SIGMA, ELL, NOISE)
    return _refs[key]


def _hold_against_fresh(actx, fctx, X, y, Xs, J0, kern, ard, lml_a, lml_f, tag, gradients=None, ratio_bar=2):
    """X, y: the surviving points, fitted afresh in fctx; actx holds the result of the removal.  ratio_bar None: the
    factor's ratio is printed only (sequences)."""
    S = _kernel_matrix(fctx, kern, X, ard)
    Ga, Gf = actx.factor(), fctx.factor()
    ra, rf = _factor_ratio(S, Ga, J0), _factor_ratio(S, Gf, J0)
    e_lml = abs(lml_a - lml_f) / abs(lml_f)
    e_m, e_diag = relmax(actx.m(), fctx.m()), relmax(actx.diag(), fctx.diag())
    e_alpha = relmax(actx.alpha(), fctx.alpha())
    mu_a, sd_a = actx.predict(Xs)
    mu_f, sd_f = fctx.predict(Xs)
    e_mu, e_sd = np.max(np.abs(mu_a - mu_f)), np.max(np.abs(sd_a - sd_f))
    print("%s: factor %.4f (fresh %.4f; bar %s)  lml %.1e  m %.1e  diag %.1e  alpha %.1e  mu %.1e  sd %.1e"
          % (tag, ra, rf, ratio_bar, e_lml, e_m, e_diag, e_alpha, e_mu, e_sd))
    assert np.all(np.isfinite(Ga)) and actx.N == X.shape[0] == actx.layout()["N"]
    if ratio_bar is not None:
        assert ra <= ratio_bar and rf <= ratio_bar, (ra, rf)
    assert e_lml <= LML_RTOL and e_m <= M_RTOL and e_diag <= DIAG_RTOL and e_alpha <= ALPHA_RTOL
    assert e_mu <= MU_ATOL and e_sd <= SD_ATOL
    if gradients is None:
        return
    ref = _scales(gradients, X, y, X.shape[1], kern, ard)
    ga, gf = actx.lml_grad_ard(), fctx.lml_grad_ard()
    e_r = np.max(np.abs(ga[0] - gf[0]) / ref["s_r"])
    e_g = [abs(ga[i] - gf[i]) / ref[s] for i, s in ((1, "s_l"), (2, "s_sigma"), (3, "s_noise"))]
    la, lf = actx.loo(), fctx.loo()
    e_lmu = np.max(np.abs(la[0] - lf[0]))
    e_lvar = np.max(np.abs(la[1] - lf[1]) / lf[1])
    e_lp = np.max(np.abs(la[2] - lf[2]) / np.maximum(1.0, np.abs(lf[2])))
    e_tot = abs(la[3] - lf[3]) / np.sum(np.abs(lf[2]))
    print("%s: grad error / scale r %.1e l %.1e sigma %.1e noise %.1e;  loo mu %.1e var %.1e logp %.1e total %.1e"
          % (tag, e_r, e_g[0], e_g[1], e_g[2], e_lmu, e_lvar, e_lp, e_tot))
    assert e_r <= GRAD_RTOL and max(e_g) <= GRAD_RTOL
    assert e_lmu <= 1e-10 * max(1.0, np.max(np.abs(y))) and e_lvar <= 1e-10 and e_lp <= 1e-10 and e_tot <= LML_RTOL


def _reset(*ctxs):
    for c in ctxs:
        _configure(c, "rbf")
        c.set_lengthscales(None)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_remove_matches_a_fresh_fit(actx, fctx, case):
    N, idx, d, kern, ard, fused = case
    X, y, Xs = _problem(N, d)
    r = R_ARD[:d] if ard else None
    keep = _survivors(N, idx)
    J0 = min(idx) // 128 * 128
    _configure(actx, kern, fused)
    _configure(fctx, kern, fused)
    try:
        actx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=r)
        lay = actx.layout()
        lead = actx.factor(0, J0, 0, J0)
        lml_a = actx.remove(idx)
        after = actx.layout()
        assert after["N"] == N - len(idx) and after["Np"] == (N - len(idx) + 127) // 128 * 128
        assert (after["ld"], after["rows"]) == (lay["ld"], lay["rows"]), "a removal keeps the allocation's shape"
        assert np.array_equal(actx.factor(0, J0, 0, J0), lead), "the leading J0 x J0 block is the resident one"
        lml_f = fctx.fit(X[keep], y[keep], SIGMA, ELL, NOISE, lengthscales=r)
        # the gradients wherever the dense mirror's scales are cheap and defined
        grads = (N, tuple(idx), d, kern, ard) if 100 <= keep.size <= 700 else None
        _hold_against_fresh(actx, fctx, X[keep], y[keep], Xs, J0, kern, ard, lml_a, lml_f, "remove " + _id(case), grads)
    finally:
        _reset(actx, fctx)


def test_composite_kernel(actx, fctx):
    """kind 3, which gpmi_append refuses: no element of K is evaluated, so the removal serves it.  The first 200 points
    of the CO2 fixture of tests/test_co2_grad_gpu.py."""
    import co2_grad_ref as CR
    from conftest import golden
    g = golden("kernels_bo_co2")
    th, X, y = g["co2_theta"], g["co2_X"][:200], g["co2_y"][:200]
    idx = [0, 77, 150, 199]
    keep = _survivors(200, idx)
    try:
        for c in (actx, fctx):
            c.set_kernel("co2", th)
        actx.fit(X, y, 1.0, 1.0, CR.NOISE, lengthscales=None)
        lml_a = actx.remove(idx)
        lml_f = fctx.fit(X[keep], y[keep], 1.0, 1.0, CR.NOISE, lengthscales=None)
        S = fctx.cov("co2", X[keep], X[keep], th) + CR.NOISE * np.eye(keep.size)
        ra, rf = R.potrf_ratio(S, actx.factor()), R.potrf_ratio(S, fctx.factor())
        e = (abs(lml_a - lml_f) / abs(lml_f), relmax(actx.m(), fctx.m()), relmax(actx.diag(), fctx.diag()),
             relmax(actx.alpha(), fctx.alpha()))
        print("composite kernel N=200 k=4: factor %.4f (fresh %.4f; bar 2)  lml %.1e  m %.1e  diag %.1e  alpha %.1e" % ((ra, rf) + e))
        assert ra <= 2 and rf <= 2
        assert e[0] <= LML_RTOL and e[1] <= M_RTOL and e[2] <= DIAG_RTOL and e[3] <= ALPHA_RTOL
        with pytest.raises(ValueError, match="composite kernel"):       # the other direction stays refused
            actx.append(X[:1] + 0.5, y[:1])
    finally:
        _reset(actx, fctx)


def test_backward_solve_before_a_removal_changes_no_bit(actx):
    """alpha first: the block-upper tiles of the diagonal blocks then hold the blocks' inverses, which the sweep must not
    read as part of L -- the result is the one without that call, bit for bit"""
    N, idx = 300, [3, 130, 131, 270]
    X, y, _ = _problem(N, 8)
    out = []
    for solve_first in (False, True):
        actx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
        if solve_first:
            assert np.all(np.isfinite(actx.alpha()))
        lml = actx.remove(idx)
        out.append((lml, actx.factor(), actx.m(), actx.alpha()))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


def test_the_same_removal_gives_the_same_bits(actx, fctx):
    N, idx = 1100, [1, 500, 640, 1099] + list(range(700, 720))
    X, y, _ = _problem(N, 8)
    out = []
    for c in (actx, fctx, actx):
        c.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
        lml = c.remove(idx)
        out.append((lml, c.factor(), c.m()))
    for o in out[1:]:
        assert o[0] == out[0][0] and np.array_equal(o[1], out[0][1]) and np.array_equal(o[2], out[0][2])


@pytest.mark.parametrize("route", [1, 0])
def test_append_after_a_removal(actx, fctx, route):
    """the stored 16 x 16 inverses of the new diagonal tiles: the skinny append's sweep, trsm128 behind the padded one and
    behind predict, and the backward solve all read them"""
    N, idx, k = 300, [0, 17, 128, 140, 299], 3
    X, y, Xs = _problem(N + k, 8)
    keep = _survivors(N, idx)
    order = np.concatenate([keep, np.arange(N, N + k)])
    _configure(actx, "rbf", route=route)
    try:
        actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
        actx.remove(idx)
        mu, sd = actx.predict(Xs)
        assert np.all(np.isfinite(mu)) and np.all(np.isfinite(sd))
        lml_a = actx.append(X[N:], y[N:])
        assert actx.layout()["route"] == route
        lml_f = fctx.fit(X[order], y[order], SIGMA, ELL, NOISE, lengthscales=None)
        _hold_against_fresh(actx, fctx, X[order], y[order], Xs, 0, "rbf", False, lml_a, lml_f,
                            "append (route %d) after a removal" % route)
    finally:
        _reset(actx)


def test_append_then_remove_returns_to_the_fit(actx, fctx):
    N, k = 300, 5
    X, y, Xs = _problem(N + k, 8)
    try:
        actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
        actx.append(X[N:], y[N:])
        lml_a = actx.remove(np.arange(N, N + k)[::-1])
        lml_f = fctx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
        _hold_against_fresh(actx, fctx, X[:N], y[:N], Xs, 256, "rbf", False, lml_a, lml_f, "append 5, remove them")
    finally:
        _reset(actx)


def test_130_single_removals(actx, fctx):
    """130 removals of index 0 from N = 430: every one shifts everything; held by m, diag, alpha, the LML and the
    predictions, the factor's ratio printed"""
    N, steps = 430, 130
    X, y, Xs = _problem(N, 8)
    actx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
    for i in range(steps):
        lml_a = actx.remove(0)
        assert actx.N == N - i - 1
    lml_f = fctx.fit(X[steps:], y[steps:], SIGMA, ELL, NOISE, lengthscales=None)
    _hold_against_fresh(actx, fctx, X[steps:], y[steps:], Xs, 0, "rbf", False, lml_a, lml_f, "130 single removals",
                        ratio_bar=None)


def test_130_sliding_window_steps(actx, fctx):
    """N = 300 with reserve 128 and the spare buffer kept: the layout is unchanged from the second step on, and the
    window matches a fresh fit of its points at the end"""
    from gaussian_process_amd import GP_regression as G
    N, steps = 300, 130
    X, y, Xs = _problem(N + steps, 8)
    _configure(actx, "rbf", reserve=128, spare=1)
    try:
        actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
        shapes = []
        for i in range(steps):
            lml_a = G.slide_window(X[N + i:N + i + 1], y[N + i:N + i + 1], ctx=actx)
            lay = actx.layout()
            assert lay["N"] == N
            shapes.append((lay["ld"], lay["rows"]))
        assert len(set(shapes[1:])) == 1, shapes
        lml_f = fctx.fit(X[steps:], y[steps:], SIGMA, ELL, NOISE, lengthscales=None)
        _hold_against_fresh(actx, fctx, X[steps:], y[steps:], Xs, 0, "rbf", False, lml_a, lml_f, "130 window steps",
                            ratio_bar=None)
    finally:
        _reset(actx)


def test_refusals_change_nothing(actx):
    from gaussian_process_amd import GPContext, _lib
    N = 150
    X, y, _ = _problem(N + 2, 8)
    with GPContext(0) as c:
        with pytest.raises(ValueError, match="no factorisation resident"):
            c.remove([0])
        c.set_train(X[:N], y[:N])
        with pytest.raises(ValueError, match="no factorisation resident"):
            c.remove([0])
        assert c.layout()["N"] == N
        labels = np.where(y[:N] > 0, 1.0, -1.0)
        c.laplace_fit(X[:N], labels, SIGMA, ELL)
        f0 = c.laplace_predict(X[N:])
        with pytest.raises(ValueError, match="no factorisation resident"):
            c.remove([0])
        assert all(np.array_equal(a, b) for a, b in zip(c.laplace_predict(X[N:]), f0)) and c.N == N
        c.sparse_fit(X[:N], y[:N], X[:40] + 0.01, SIGMA, ELL, NOISE)
        s0 = c.sparse_predict(X[N:])
        with pytest.raises(ValueError, match="no factorisation resident"):
            c.remove([0])
        assert all(np.array_equal(a, b) for a, b in zip(c.sparse_predict(X[N:]), s0))
    actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
    G0, a0, lay = actx.factor(), actx.alpha(), actx.layout()
    G0 = actx.factor()                                   # after the backward solve, as the comparisons below read it
    for idx in ([], list(range(N)), list(range(N + 1)), [-1], [N], [3, N], [5, 9, 5]):
        with pytest.raises(ValueError, match="gpmi_remove"):
            actx.remove(idx)
        assert actx.N == N and actx.layout() == lay
        assert np.array_equal(actx.factor(), G0) and np.array_equal(actx.alpha(), a0)
    lml = C.c_double()
    assert actx._lib.gpmi_remove(actx._h, None, 1, C.byref(lml)) == _lib.GPMI_ERR_BAD_ARG
    assert actx.layout() == lay and np.array_equal(actx.factor(), G0)
    with pytest.raises(ValueError):
        actx.remove([0.5])
    assert np.isfinite(actx.remove([3, 1])) and actx.N == N - 2


def test_posterior_factor_asks_for_a_new_prediction(actx, fctx):
    """a test set, v and the posterior-sample factor before a removal: afterwards v is gone, post_chol is refused with the
    text of a context that has not predicted yet, and a new prediction serves the reduced fit"""
    N, idx = 200, [4, 150]
    X, y, Xs = _problem(N, 8)
    keep = _survivors(N, idx)
    actx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
    actx.predict(Xs)
    actx.post_chol(1e-6)
    actx.remove(idx)
    with pytest.raises(ValueError, match="run gpmi_predict first"):
        actx.post_chol(1e-6)
    mu, sd = actx.predict_resident()
    fctx.fit(X[keep], y[keep], SIGMA, ELL, NOISE, lengthscales=None)
    mu_f, sd_f = fctx.predict(Xs)
    assert np.max(np.abs(mu - mu_f)) <= MU_ATOL and np.max(np.abs(sd - sd_f)) <= SD_ATOL
    assert np.allclose(actx.post_chol(1e-6), fctx.post_chol(1e-6), rtol=0, atol=1e-6)
    # the one-pass fit with the riding posterior factor (the y row behind the test rows), then a removal
    actx.set_train(X, y)
    actx.set_test(Xs)
    actx.fit_predict_sample_resident(SIGMA, ELL, NOISE, 1e-6)
    lml_a = actx.remove(idx)
    with pytest.raises(ValueError, match="run gpmi_predict first"):
        actx.post_chol(1e-6)
    lml_f = fctx.fit(X[keep], y[keep], SIGMA, ELL, NOISE, lengthscales=None)
    _hold_against_fresh(actx, fctx, X[keep], y[keep], Xs, 0, "rbf", False, lml_a, lml_f,
                        "removal behind the augmented one-pass fit")


def test_lml_batch_sees_the_reduced_training_set(actx, fctx):
    N, idx = 300, [0, 299, 128]
    X, y, _ = _problem(N, 8)
    keep = _survivors(N, idx)
    actx.set_option("lanes", 2)
    try:
        actx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
        triples = np.array([[ELL, SIGMA, NOISE], [2.0, 1.0, 1e-2], [1.0, 0.9, 2e-2]])
        actx.lml_batch(triples)                              # the lanes now hold the 300 points
        actx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
        actx.remove(idx)
        got, status = actx.lml_batch(triples)
        want = [fctx.fit(X[keep], y[keep], s, l, nv, lengthscales=None) for l, s, nv in triples]
        assert np.all(status == 0)
        assert np.max(np.abs(got - want) / np.abs(want)) <= LML_RTOL
    finally:
        actx.set_option("lanes", 0)


def test_remove_observations_wrapper(actx, fctx):
    from gaussian_process_amd import GP_regression as G
    N, idx = 140, [139, 0, 70]
    X, y, _ = _problem(N, 8)
    keep = _survivors(N, idx)
    actx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
    got = G.remove_observations(idx, ctx=actx)
    want = fctx.fit(X[keep], y[keep], SIGMA, ELL, NOISE, lengthscales=None)
    assert abs(got - want) <= LML_RTOL * abs(want) and actx.N == N - 3
