"""The resident-state rule of tests/state_table.py replayed through the library: after every event of every sequence each
group of consumers either succeeds or is refused with its message, as the table says.

N = 130 (two tiles with padding: the smallest size where Np != N and the factor has an off-diagonal tile), d = 2, n = 5
test points, m = 40 inducing points, C = 3.  The fits and predictions go through the C entry points on the RESIDENT
training set (the Python wrappers upload a new one, which is an event of its own), so one target vector serves all of
them: y = 1 everywhere is a label of the binary classifier and of the softmax one, and a regression target."""
import ctypes as C

import numpy as np
import pytest

import state_table as T

pytestmark = pytest.mark.gpu

N, D, N_TEST, M, CLASSES = 130, 2, 5, 40, 3
SIGMA, ELL, NOISE, JITTER = 1.0, 1.0, 1e-2, 1e-6
_rng = np.random.default_rng(130)
X = _rng.uniform(0.0, 4.0, size=(N, D))
Y = np.ones(N)
Z = np.ascontiguousarray(X[:M] + 0.01)
XS = _rng.uniform(0.0, 4.0, size=(N_TEST, D))
XS2 = _rng.uniform(0.0, 4.0, size=(N_TEST, D))


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: kernel, lengthscales and ld_pad are context state"""
    from gaussian_process_amd import GPContext
    c = GPContext(0)
    yield c
    c.close()


def _out(*shape):
    from gaussian_process_amd._lib import ptr
    a = np.empty(shape)
    return a, ptr(a)


def _newton_outputs():
    return C.byref(C.c_double()), C.byref(C.c_int()), C.byref(C.c_int())


def _event(c, ev):
    """the library call behind an event of the table; raises what the library raises"""
    from gaussian_process_amd._lib import check, ptr
    L, h = c._lib, c._h
    if ev == "set_train":
        c.set_train(X, Y)
    elif ev == "set_test":
        check(L.gpmi_set_test(h, ptr(XS), N_TEST))
    elif ev == "factorize":
        c.factorize(SIGMA, ELL, NOISE)
    elif ev == "fit_predict":
        check(L.gpmi_fit_predict_resident(h, SIGMA, ELL, NOISE, C.byref(C.c_double()), C.byref(C.c_int64()), _out(N_TEST)[1],
                                          _out(N_TEST)[1], 1))
    elif ev == "fit_predict_sample":
        check(L.gpmi_fit_predict_sample_resident(h, SIGMA, ELL, NOISE, JITTER, C.byref(C.c_double()), C.byref(C.c_int64()),
                                                 _out(N_TEST)[1], _out(N_TEST)[1], 1, None))
    elif ev == "predict":
        check(L.gpmi_predict_resident(h, _out(N_TEST)[1], _out(N_TEST)[1], 1))
    elif ev == "laplace_fit":
        check(L.gpmi_laplace_fit(h, SIGMA, ELL, 1e-10, 20, *_newton_outputs(), _out(N)[1]))
    elif ev == "softmax_fit":
        check(L.gpmi_softmax_fit(h, CLASSES, SIGMA, ELL, 1e-10, 20, *_newton_outputs(), _out(CLASSES, N)[1]))
    elif ev == "sparse_fit":
        check(L.gpmi_sparse_fit(h, ptr(Z), M, SIGMA, ELL, NOISE, 1e-6, 0, C.byref(C.c_double()), C.byref(C.c_int64())))
    elif ev in ("laplace_predict", "softmax_predict", "sparse_predict", "post_chol"):
        _consume(c, {"laplace_predict": "laplace", "softmax_predict": "softmax", "sparse_predict": "sparse",
                     "post_chol": "post"}[ev])
    elif ev == "set_kernel":
        c.set_kernel("lin", 0.5)
    elif ev == "set_lengthscales":
        c.set_lengthscales(np.array([1.5, 0.7]))
    elif ev == "ld_pad":
        c.set_option("ld_pad", 512)
    else:
        raise AssertionError(ev)


def _consume(c, group):
    """one consumer of the group; none of them changes what the groups accept"""
    from gaussian_process_amd._lib import check
    L, h = c._lib, c._h
    if group == "regression":
        check(L.gpmi_get_alpha(h, _out(N)[1]))
    elif group == "post":
        check(L.gpmi_post_chol(h, JITTER, _out(N_TEST, N_TEST)[1], C.byref(C.c_int64())))
    elif group == "laplace":
        check(L.gpmi_laplace_predict_resident(h, _out(N_TEST)[1], _out(N_TEST)[1], _out(N_TEST)[1]))
    elif group == "softmax":
        check(L.gpmi_softmax_predict_resident(h, _out(N_TEST, CLASSES)[1], _out(N_TEST, CLASSES, CLASSES)[1], 0, None, None))
    elif group == "sparse":
        check(L.gpmi_sparse_predict_resident(h, _out(N_TEST)[1], _out(N_TEST)[1], 1))
    else:
        raise AssertionError(group)


def _replay(c, seq):
    model = T.Model()
    for k, ev in enumerate(seq):
        where = "%s: event %d (%s)" % (" ".join(seq), k + 1, ev)
        if model.apply(ev):
            _event(c, ev)
        else:
            with pytest.raises(ValueError):
                _event(c, ev)
        ok = model.accepted()
        for group in ("regression", "post", "laplace", "softmax", "sparse"):
            # a prediction asks for its fit first and for the test set second
            text = None if group in ok else T.GROUPS[group]
            if text is None and group in ("laplace", "softmax", "sparse") and "test" not in ok:
                text = T.GROUPS["test"]
            if text is None:
                _consume(c, group)
            else:
                with pytest.raises(ValueError, match=text):
                    _consume(c, group)
                    pytest.fail("%s: %s was accepted" % (where, group))


@pytest.mark.parametrize("seq", T.sequences(), ids=lambda s: "-".join(s))
def test_sequence(ctx, seq):
    from gaussian_process_amd import GPContext
    try:
        if seq[0] == "set_train":
            _replay(ctx, seq)
        else:                               # nothing resident at all: a context that never saw a training set
            with GPContext(0) as empty:
                _replay(empty, seq)
    finally:
        ctx.set_kernel("rbf")
        ctx.set_option("ld_pad", 544)
        ctx.set_lengthscales(None)


@pytest.mark.parametrize("first", ["factorize", "fit_predict_sample"])
def test_the_kept_posterior_factor_is_never_another_test_sets(ctx, first):
    """the factor kept for one v (in its own buffer, or behind L) is not served for the v of the next test set: the
    second answer has the bits of a context that never saw the first test set"""
    from gaussian_process_amd import GPContext
    ctx.set_train(X, Y)
    ctx.set_test(XS)
    _event(ctx, first)
    if first == "factorize":
        ctx.predict_resident()
    L1 = ctx.post_chol(JITTER)
    assert np.array_equal(ctx.post_chol(JITTER), L1)
    ctx.predict(XS2)
    L2 = ctx.post_chol(JITTER)
    with GPContext(0) as other:
        other.set_train(X, Y)
        other.set_test(XS2)
        _event(other, first)                # the same factorisation, with the second test set from the start
        other.predict_resident()
        want = other.post_chol(JITTER)
    assert np.array_equal(L2, want) and not np.array_equal(L2, L1)
