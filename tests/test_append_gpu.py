"""GPContext.append (gpmi_append) against a fresh fit of the concatenated data in a second context: the factor at the
componentwise bar of the panel kernels (tests/panel_ref.py: |K_y - L L^T| <= 2 n u |L| |L^T|), the LML, m, alpha and
diag(L) at the bars of tests/test_parity_gpu.py, and predict, lml_grad_ard and loo at the bars of their own GPU tests.
The (N, k) pairs cover N0 = 0, an aligned N, an append inside the padding, one that crosses a tile, the skinny route at
its largest k, the first padded k, several border tiles, sweeps over several outer blocks; every k <= 16 pair runs on
both routes (option "append_skinny" 0 and 1).  Then the sequences: 130 single points from N = 120 (in-place growth, the
reallocations, the y-row move; none with "reserve"), a backward solve before an append, a far point, a test set and its
posterior factor before an append, what is refused, the failed pivot, and first-generation factors ("panel_fused" 0).

Noise is 1e-2, so both sides sit well inside the bars.  Every case prints its figures.  Above 700 points the factor's
componentwise ratio is taken on a sample of the border rows (_factor_ratio says which and why)."""
import numpy as np
import pytest

import ard_ref
import matern_ref
import panel_ref as R

pytestmark = pytest.mark.gpu

LML_RTOL, M_RTOL, ALPHA_RTOL, DIAG_RTOL = 1e-10, 1e-9, 1e-8, 1e-11      # tests/test_parity_gpu.py
MU_ATOL, SD_ATOL = 1e-9, 1e-9                                           # tests/test_parity_gpu.py
GRAD_RTOL = 1e-8              # tests/test_ard_gpu.py, tests/test_loo_gpu.py: relative to the terms that cancel
SIGMA, ELL, NOISE = 1.2, 1.5, 1e-2
R_ARD = np.array([0.7, 1.0, 1.6, 0.9, 2.5, 1.2, 0.8, 1.1])

PAIRS = [(1, 1), (128, 1), (200, 1), (255, 2), (256, 16), (300, 17), (300, 200), (1100, 1), (1100, 1000), (2300, 5)]
SMALL = [(N, k) for N, k in PAIRS if N + k <= 700]
# every pair at d = 8 with the squared exponential, each k <= 16 pair on both routes; the other settings on the small pairs
CASES = ([(N, k, 8, "rbf", route, False) for N, k in PAIRS for route in ((0, 1) if k <= 16 else (-1,))] +
         [(N, k, d, kern, -1, False) for N, k in SMALL for d, kern in ((1, "rbf"), (8, "matern52"), (1, "matern52"))] +
         [(255, 2, 8, "rbf", 1, True), (300, 17, 8, "rbf", -1, True), (256, 16, 8, "matern52", 1, True)])


@pytest.fixture(scope="module")
def actx():
    """the context that appends; options, kernel and lengthscales are context state, so it is this module's own"""
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


def _problem(N1, d):
    if (N1, d) not in _data:
        X, y = ard_ref.problem(N1, d, seed=1000 + N1 + d)
        rng = np.random.default_rng(N1 + d)
        Xs = rng.uniform(0.0, 4.0, size=(40, d))
        X.setflags(write=False)
        y.setflags(write=False)
        _data[N1, d] = (X, y, Xs)
    return _data[N1, d]


_refs = {}


def _scales(N1, d, kern, ard):
    """the cancellation scales of the gradients from the dense mirror, once per data set"""
    key = (N1, d, kern, ard)
    if key not in _refs:
        X, y, _ = _problem(N1, d)
        r = R_ARD[:d] if ard else np.ones(d)
        if kern == "rbf":
            _refs[key] = ard_ref.lml_and_grad(X, y, r, SIGMA, ELL, NOISE)
        else:
            _refs[key] = matern_ref.lml_and_grad(X, y, r, 2.5, SIGMA, ELL, NOISE)
    return _refs[key]


def _ratio_rows(S, G, rows):
    """panel_ref.potrf_ratio on the given rows only (rows are independent in it): worst |S - L L^T|_ij / (n u (|L| |L^T|)_ij),
    j <= i, the residual in long double, the sums cut at the last column of j's 128-column block"""
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


def _factor_ratio(S, G, N, k):
    """panel_ref.potrf_ratio on the whole factor up to 700 points.  Beyond (the pairs (1100, 1), (1100, 1000) and
    (2300, 5)) the assertion is SAMPLED: the residual is a long-double product without BLAS, about 160 Mflop/s here, so
    all 1076 border rows of (1100, 1000) would take 15 s per factor and a test case is allowed a few.  Checked are rows
    of the border only (the rows below N0 are the resident ones bit for bit, which the test asserts): all of them up to
    `cap`, else the first and the last, every new row when k <= 16, and a seeded sample up to cap -- 64 rows for k <= 16
    (the border has at most 144), 128 otherwise, spread over every tile of the border.  m, diag(L) and alpha against the
    fresh fit cover every row."""
    N1 = S.shape[0]
    if N1 <= 700:
        return R.potrf_ratio(S, G)
    rows = np.arange(N // 128 * 128, N1)
    cap = 64 if k <= 16 else 128
    if rows.size > cap:
        keep = {int(rows[0]), int(rows[-1])} | (set(range(N, N1)) if k <= 16 else set())
        rng = np.random.default_rng(N1)
        keep |= set(int(v) for v in rng.choice(rows, cap - len(keep), replace=False))
        rows = np.array(sorted(keep))
    return _ratio_rows(S, G, rows)


def _configure(c, kern, route=-1, fused=1, reserve=0):
    c.set_kernel(kern)
    c.set_option("append_skinny", route)
    c.set_option("panel_fused", fused)
    c.set_option("reserve", reserve)


def _kernel_matrix(c, kern, X, ard):
    Z = X / R_ARD[:X.shape[1]] if ard else X
    K = c.rbf(Z, Z, SIGMA, ELL) if kern == "rbf" else c.cov(kern, Z, Z, SIGMA, ELL)
    K[np.diag_indices_from(K)] += NOISE
    return K


def _hold_against_fresh(actx, fctx, X, y, Xs, N, k, kern, ard, lml_a, lml_f, tag, gradients=True):
    """everything the issue lists, appended context against fresh context"""
    N1, d = X.shape
    S = _kernel_matrix(fctx, kern, X, ard)
    Ga, Gf = actx.factor(), fctx.factor()
    ra, rf = _factor_ratio(S, Ga, N, k), _factor_ratio(S, Gf, N, k)
    e_lml = abs(lml_a - lml_f) / abs(lml_f)
    e_m, e_diag = relmax(actx.m(), fctx.m()), relmax(actx.diag(), fctx.diag())
    e_alpha = relmax(actx.alpha(), fctx.alpha())
    mu_a, sd_a = actx.predict(Xs)
    mu_f, sd_f = fctx.predict(Xs)
    e_mu, e_sd = np.max(np.abs(mu_a - mu_f)), np.max(np.abs(sd_a - sd_f))
    print("%s: factor %.4f (fresh %.4f; bar 2)  lml %.1e  m %.1e  diag %.1e  alpha %.1e  mu %.1e  sd %.1e"
          % (tag, ra, rf, e_lml, e_m, e_diag, e_alpha, e_mu, e_sd))
    assert np.all(np.isfinite(Ga))
    assert ra <= 2 and rf <= 2, (ra, rf)
    assert e_lml <= LML_RTOL and e_m <= M_RTOL and e_diag <= DIAG_RTOL and e_alpha <= ALPHA_RTOL
    assert e_mu <= MU_ATOL and e_sd <= SD_ATOL
    if not gradients:
        return
    ref = _scales(N1, d, kern, ard)
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


@pytest.mark.parametrize("N,k,d,kern,route,ard", CASES)
def test_append_matches_a_fresh_fit(actx, fctx, N, k, d, kern, route, ard):
    X, y, Xs = _problem(N + k, d)
    r = R_ARD[:d] if ard else None
    _configure(actx, kern, route)
    _configure(fctx, kern)
    try:
        actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=r)
        N0 = N // 128 * 128
        lead = actx.factor(0, N0, 0, N0)
        lml_a = actx.append(X[N:], y[N:])
        assert actx.N == N + k and actx.layout()["N"] == N + k
        # the skinny route wherever it is allowed (k <= 16, a fused factor, something to sweep) unless the option says never
        assert actx.layout()["route"] == (1 if k <= 16 and N >= 128 and route != 0 else 0)
        assert np.array_equal(actx.factor(0, N0, 0, N0), lead), "the leading N0 x N0 block is the resident one"
        lml_f = fctx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=r)
        tag = "append N=%d k=%d d=%d %s route %d%s" % (N, k, d, kern, route, " ard" if ard else "")
        _hold_against_fresh(actx, fctx, X, y, Xs, N, k, kern, ard, lml_a, lml_f, tag)
    finally:
        for c in (actx, fctx):
            _configure(c, "rbf")
            c.set_lengthscales(None)


@pytest.mark.parametrize("N,k,route", [(300, 17, -1), (300, 3, 1), (300, 200, -1)])
def test_device_against_the_mirror(actx, N, k, route):
    """tests/append_ref.py (held on the CPU to half the factor's bar and half the LML's) runs the device's recurrences in
    float64 on the device's own K: the appended factor's diagonal and m agree with the mirror's at the bars the appended
    fit is held to against a fresh one (DIAG_RTOL, M_RTOL), the LML at LML_RTOL, and the whole lower triangle at M_RTOL"""
    import append_ref as AR
    X, y, _ = _problem(N + k, 8)
    _configure(actx, "rbf", route)
    try:
        S = _kernel_matrix(actx, "rbf", X, False)
        G0, m0 = AR.fit(S[:N, :N], y[:N])
        G1, m1 = AR.append(G0, m0, N, S, y)
        actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
        lml = actx.append(X[N:], y[N:])
        N1 = N + k
        e_diag = relmax(actx.diag(), np.diag(G1)[:N1])
        e_m = relmax(actx.m(), m1[:N1])
        e_f = relmax(actx.factor(), np.tril(G1[:N1, :N1]))
        e_lml = abs(lml - AR.lml(G1, m1, N1)) / abs(lml)
        print("device against mirror N=%d k=%d route %d: diag %.1e  m %.1e  factor %.1e  lml %.1e" % (N, k, route, e_diag, e_m, e_f, e_lml))
        assert e_diag <= DIAG_RTOL and e_m <= M_RTOL and e_f <= M_RTOL and e_lml <= LML_RTOL
    finally:
        _configure(actx, "rbf")


def test_routes_differ_only_in_rounding(actx):
    """both routes on one input: the same leading block, and factors that agree to the bar of diag(L)"""
    N, k = 2300, 5
    X, y, _ = _problem(N + k, 8)
    out = []
    for route in (0, 1):
        _configure(actx, "rbf", route)
        actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
        actx.append(X[N:], y[N:])
        assert actx.layout()["route"] == route
        out.append(actx.factor(N, N + k, 0, N + k))
    _configure(actx, "rbf")
    assert relmax(out[1], out[0]) <= 1e-9


@pytest.mark.parametrize("reserve", [0, 200])
def test_130_single_points(actx, fctx, reserve):
    """130 appends of one point from N = 120: inside the padding up to 128, a reallocation with the y-row move at 129 and
    in-place growth behind it -- and 10 more, which cross 256 and reallocate again.  With reserve = 200 the first fit is
    sized for 320 points and nothing moves until then: the leading dimension and the rows of A stay what they were."""
    N, steps = 120, 140
    X, y, Xs = _problem(N + steps, 8)
    _configure(actx, "rbf", -1, reserve=reserve)
    _configure(fctx, "rbf")
    try:
        actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
        first = actx.layout()
        assert first["ld"] == (128 if reserve == 0 else 384) + 544 and first["rows"] == (128 if reserve == 0 else 384) + 128
        moves, prev = 0, first
        for i in range(N, N + steps):
            lml_a = actx.append(X[i], y[i])             # a single point as a 1-D row
            lay = actx.layout()
            assert lay["N"] == i + 1 and lay["Np"] == (i + 1 + 127) // 128 * 128
            moves += (lay["ld"], lay["rows"]) != (prev["ld"], prev["rows"])
            prev = lay
            if i + 1 == N + 130:
                assert moves == (1 if reserve == 0 else 0)
                lml_f = fctx.fit(X[:i + 1], y[:i + 1], SIGMA, ELL, NOISE, lengthscales=None)
                _hold_against_fresh(actx, fctx, X[:i + 1], y[:i + 1], Xs, N, 130, "rbf", False, lml_a, lml_f,
                                    "130 single points, reserve %d" % reserve, gradients=False)
        assert moves == (2 if reserve == 0 else 0)
        if reserve:
            assert (prev["ld"], prev["rows"]) == (first["ld"], first["rows"])
        lml_f = fctx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
        _hold_against_fresh(actx, fctx, X, y, Xs, N, steps, "rbf", False, lml_a, lml_f,
                            "140 single points, reserve %d" % reserve)
    finally:
        _configure(actx, "rbf")


def test_the_lml_of_each_step_is_the_fresh_one(actx, fctx):
    """the value append returns, step by step across the tile boundary"""
    N = 124
    X, y, _ = _problem(N + 8, 8)
    _configure(actx, "rbf")
    actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
    for i in range(N, N + 8):
        got = actx.append(X[i:i + 1], y[i:i + 1])
        want = fctx.fit(X[:i + 1], y[:i + 1], SIGMA, ELL, NOISE, lengthscales=None)
        assert abs(got - want) <= LML_RTOL * abs(want), (i, got, want)


@pytest.mark.parametrize("route", [0, 1])
def test_backward_solve_before_an_append(actx, fctx, route):
    """alpha first: the block-upper tiles of the diagonal blocks then hold the blocks' inverses, which neither route may
    read as part of L, and which the next backward solve has to make again for the border"""
    N, k = 300, 3
    X, y, Xs = _problem(N + k, 8)
    _configure(actx, "rbf", route)
    try:
        actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
        a0 = actx.alpha()
        assert np.all(np.isfinite(a0))
        lml_a = actx.append(X[N:], y[N:])
        lml_f = fctx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
        _hold_against_fresh(actx, fctx, X, y, Xs, N, k, "rbf", False, lml_a, lml_f, "alpha before append, route %d" % route)
        assert relmax(actx.alpha(), fctx.alpha()) <= ALPHA_RTOL          # and again, from the inverses just made
    finally:
        _configure(actx, "rbf")


@pytest.mark.parametrize("N,k,route,ell", [(200, 1, 1, ELL), (200, 1, 0, ELL), (300, 17, -1, ELL), (200, 1, 1, 400.0),
                                           (200, 1, 0, 400.0)])
def test_a_point_far_from_the_old_box(actx, fctx, N, k, route, ell):
    """new points 1e3 away from the box of the old ones: the bounding box lets the K build drop its exp domain test, so a
    box that was not extended gives wrong rows of K.  L[i][0] = K[i][0] / L[0][0] with nothing added, in the append and
    in the fresh fit alike: column 0 of the new rows of the factor is the K row's, bit for bit.  At l = 1.5 the exp
    argument is far outside the domain (K is 0 exactly), at l = 400 it is an ordinary value."""
    X, y, Xs = _problem(N + k, 2)
    X = np.array(X)
    X[N:] += 1e3
    _configure(actx, "rbf", route)
    try:
        actx.fit(X[:N], y[:N], SIGMA, ell, NOISE, lengthscales=None)
        lml_a = actx.append(X[N:], y[N:])
        lml_f = fctx.fit(X, y, SIGMA, ell, NOISE, lengthscales=None)
        col_a, col_f = actx.factor(N, N + k, 0, 1), fctx.factor(N, N + k, 0, 1)
        K0 = fctx.rbf(X[N:], X[:1], SIGMA, ell)
        print("far point N=%d k=%d route %d l=%g: K[N][0] = %.3e, L[N][0] = %.3e" % (N, k, route, ell, K0[0, 0], col_a[0, 0]))
        assert np.array_equal(col_a, col_f)
        assert np.all(K0 == 0.0) if ell == ELL else np.all(K0 > 1e-3)
        assert abs(lml_a - lml_f) <= LML_RTOL * abs(lml_f)
        assert relmax(actx.factor(N, N + k, 0, N + k), fctx.factor(N, N + k, 0, N + k)) <= 1e-9
        assert relmax(actx.alpha(), fctx.alpha()) <= ALPHA_RTOL
    finally:
        _configure(actx, "rbf")


def test_posterior_factor_asks_for_a_new_prediction(actx, fctx):
    """a test set, v and the posterior-sample factor before an append: afterwards v is gone, post_chol is refused with the
    text of a context that has not predicted yet, and a new prediction serves the extended fit"""
    N, k = 200, 2
    X, y, Xs = _problem(N + k, 8)
    _configure(actx, "rbf")
    actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
    actx.predict(Xs)
    actx.post_chol(1e-6)
    actx.append(X[N:], y[N:])
    with pytest.raises(ValueError, match="run gpmi_predict first"):
        actx.post_chol(1e-6)
    mu, sd = actx.predict_resident()
    fctx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
    mu_f, sd_f = fctx.predict(Xs)
    assert np.max(np.abs(mu - mu_f)) <= MU_ATOL and np.max(np.abs(sd - sd_f)) <= SD_ATOL
    assert np.allclose(actx.post_chol(1e-6), fctx.post_chol(1e-6), rtol=0, atol=1e-6)
    # the one-pass fit with the riding posterior factor, then an append
    actx.set_train(X[:N], y[:N])
    actx.set_test(Xs)
    actx.fit_predict_sample_resident(SIGMA, ELL, NOISE, 1e-6)
    lml_a = actx.append(X[N:], y[N:])
    with pytest.raises(ValueError, match="run gpmi_predict first"):
        actx.post_chol(1e-6)
    lml_f = fctx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
    _hold_against_fresh(actx, fctx, X, y, Xs, N, k, "rbf", False, lml_a, lml_f, "append behind the augmented one-pass fit",
                        gradients=False)


def test_refusals_change_nothing(actx):
    """no fit, a fit of another kind, k < 1 and NaN: GPMI_ERR_BAD_ARG, and whatever was resident still is"""
    from gaussian_process_amd import GPContext
    N = 150
    X, y, _ = _problem(N + 2, 8)
    with GPContext(0) as c:
        with pytest.raises(ValueError, match="no factorisation resident"):
            c.append(X[N:], y[N:])
        c.set_train(X[:N], y[:N])
        with pytest.raises(ValueError, match="no factorisation resident"):
            c.append(X[N:], y[N:])
        assert c.layout()["N"] == N
        labels = np.where(y[:N] > 0, 1.0, -1.0)
        c.laplace_fit(X[:N], labels, SIGMA, ELL)
        f0 = c.laplace_predict(X[N:])
        with pytest.raises(ValueError, match="no factorisation resident"):
            c.append(X[N:], y[N:])
        assert all(np.array_equal(a, b) for a, b in zip(c.laplace_predict(X[N:]), f0)) and c.N == N
        c.softmax_fit(X[:N], (y[:N] > 0).astype(int), 2, SIGMA, ELL)
        with pytest.raises(ValueError, match="no factorisation resident"):
            c.append(X[N:], y[N:])
        c.sparse_fit(X[:N], y[:N], X[:40] + 0.01, SIGMA, ELL, NOISE)
        s0 = c.sparse_predict(X[N:])
        with pytest.raises(ValueError, match="no factorisation resident"):
            c.append(X[N:], y[N:])
        assert all(np.array_equal(a, b) for a, b in zip(c.sparse_predict(X[N:]), s0))
    _configure(actx, "rbf")
    lml = actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
    m0, lay = actx.m(), actx.layout()
    bad = np.array(X[N:])
    bad[1, 3] = np.nan
    for Xn, yn in ((bad, y[N:]), (X[N:], np.array([0.1, np.nan])), (np.empty((0, 8)), np.empty(0))):
        with pytest.raises(ValueError, match="gpmi_append"):
            actx.append(Xn, yn)
        assert actx.N == N and actx.layout() == lay and np.array_equal(actx.m(), m0)
    with pytest.raises(ValueError):
        actx.append(X[N:, :5], y[N:])
    assert np.isfinite(lml) and np.isfinite(actx.append(X[N:], y[N:])) and actx.N == N + 2


def test_composite_kernel_is_refused(actx):
    N = 60
    X, y, _ = _problem(N + 2, 1)
    theta = np.array([1.0, 2.0, 0.5, 3.0, 1.0, 0.4, 1.5, 0.8, 0.2, 1.1, 0.1])
    try:
        actx.set_kernel("co2", theta)
        actx.fit(X[:N], y[:N], 1.0, 1.0, NOISE, lengthscales=None)
        m0 = actx.m()
        with pytest.raises(ValueError, match="composite kernel"):
            actx.append(X[N:], y[N:])
        assert actx.N == N and np.array_equal(actx.m(), m0)
    finally:
        actx.set_kernel("rbf")


@pytest.mark.parametrize("route", [0, 1])
def test_failed_pivot_of_the_border(actx, fctx, route):
    """well-separated points, sigma = 1 and noise_var = -0.5: K is nearly the identity, K - I / 2 positive definite.  A
    new point on top of an old one makes the border pivot 0.5 - 2 < 0 (1 - .5 - (1 / sqrt(.5))^2): NOT_PD with
    bad_pivot = N + 1, the fit dropped, the extended training set resident -- factorize with noise 1e-2 succeeds on it
    and matches a fresh fit."""
    N, d = 200, 2
    g = np.arange(N)
    X = np.stack([(g % 20) * 10.0, (g // 20) * 10.0], axis=1)
    y = np.sin(g * 0.37)
    Xn, yn = X[57:58].copy(), np.array([0.25])
    _configure(actx, "rbf", route)
    try:
        actx.fit(X, y, 1.0, 1.0, -0.5, lengthscales=None)
        with pytest.raises(np.linalg.LinAlgError) as err:
            actx.append(Xn, yn)
        assert err.value.bad_pivot == N + 1
        assert actx.N == N + 1 and actx.layout()["N"] == N + 1
        with pytest.raises(ValueError, match="no factorisation resident"):
            actx.m()
        with pytest.raises(ValueError, match="no factorisation resident"):
            actx.append(Xn, yn)
        X1, y1 = np.vstack([X, Xn]), np.concatenate([y, yn])
        lml_a = actx.factorize(1.0, 1.0, 1e-2)
        lml_f = fctx.fit(X1, y1, 1.0, 1.0, 1e-2, lengthscales=None)
        assert abs(lml_a - lml_f) <= LML_RTOL * abs(lml_f)
        assert relmax(actx.m(), fctx.m()) <= M_RTOL and relmax(actx.alpha(), fctx.alpha()) <= ALPHA_RTOL
    finally:
        _configure(actx, "rbf")


@pytest.mark.parametrize("N,k", [(200, 1), (255, 2), (300, 200), (1100, 1)])
def test_first_generation_factor_takes_the_padded_route(actx, fctx, N, k):
    """option panel_fused = 0: the resident factor carries no 16 x 16 inverses, so "append_skinny" 1 still takes the padded
    route, the border is factored by the same leaves, and the same checks pass"""
    X, y, Xs = _problem(N + k, 8)
    _configure(actx, "rbf", 1, fused=0)
    _configure(fctx, "rbf", -1, fused=0)
    try:
        actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
        lml_a = actx.append(X[N:], y[N:])
        assert actx.layout()["route"] == 0
        lml_f = fctx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
        _hold_against_fresh(actx, fctx, X, y, Xs, N, k, "rbf", False, lml_a, lml_f, "first-generation N=%d k=%d" % (N, k))
    finally:
        _configure(actx, "rbf")
        _configure(fctx, "rbf")


def test_append_observations_wrapper(actx, fctx):
    from gaussian_process_amd import GP_regression as G
    N, k = 140, 3
    X, y, _ = _problem(N + k, 8)
    _configure(actx, "rbf")
    actx.fit(X[:N], y[:N], SIGMA, ELL, NOISE, lengthscales=None)
    got = G.append_observations(X[N:], y[N:], ctx=actx)
    want = fctx.fit(X, y, SIGMA, ELL, NOISE, lengthscales=None)
    assert abs(got - want) <= LML_RTOL * abs(want)
