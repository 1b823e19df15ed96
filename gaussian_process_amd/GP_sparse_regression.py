"""Sparse GP regression with inducing points on the MI355X: the counterpart of GP_regression.prediction for training
sets far beyond an N x N covariance (GPML chapter 8; Titsias 2009 for "vfe", Snelson & Ghahramani 2006 for "fitc").
The reference has no such function; the call shape follows its prediction().  The arithmetic runs through
libgpmi355x.so (gpmi_sparse_fit, gpmi_sparse_predict_resident, gpmi_sparse_grad); there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from .gp import default_context, sparse_args, split_lengthscale


def choose_inducing(X, m, seed=0):
    """m rows of X drawn without replacement on the host (np.random.default_rng(seed)), in their order in X.  No more
    than that: a random subset of clustered data is itself clustered.  It is a starting point --
    tune_hyperparms_regression.tune_hyperparms_sparse moves the inducing inputs (and the hyper-parameters) up the
    gradient of the VFE bound, sparse_bound_and_gradient returns that gradient."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be 2-dimensional, got shape %s" % (X.shape,))
    if not 1 <= int(m) <= X.shape[0]:
        raise ValueError("m must be in 1..N = %d, got %r" % (X.shape[0], m))
    idx = np.sort(np.random.default_rng(seed).choice(X.shape[0], size=int(m), replace=False))
    return np.ascontiguousarray(X[idx])


def sparse_prediction(X_train, X_test, y_train, Z, sigma, l, noise_var, method="vfe", jitter=1e-6, ctx=None):
    """Fit on (X_train, y_train) with the inducing inputs Z and predict at X_test.

    :param Z: (m, d) inducing inputs, m <= N (choose_inducing draws a random subset)
    :param sigma: output scale; l: lengthscale (scalar) or a d-vector, one lengthscale per input dimension
    :param noise_var: noise variance, > 0
    :param method: "vfe" (collapsed variational bound, the default) or "fitc"
    :return: (mu, sd, value): mean and standard deviation of the latent function at X_test, and the bound ("vfe") or
             log likelihood ("fitc") of the fit
    """
    X_train, Z, _ = sparse_args(X_train, Z, method)          # refusals that need no device come first
    l, r = split_lengthscale(l)
    ctx = ctx or default_context()
    value = ctx.sparse_fit(X_train, y_train, Z, sigma, l, noise_var, method=method, jitter=jitter, lengthscales=r)
    try:
        mu, sd = ctx.sparse_predict(X_test, want_sd=True)
    finally:
        if r is not None:
            ctx.set_lengthscales(None)                       # as every drop-in function: no lengthscales left behind
    return mu, sd, value


def sparse_bound_and_gradient(X, y, Z, sigma, l, noise_var, jitter=1e-6, ctx=None):
    """The collapsed variational bound (VFE) at the inducing inputs Z and its gradient.

    :param l: lengthscale (scalar) or a d-vector, one lengthscale per input dimension, as in sparse_prediction
    :return: (value, grad): grad is the dict of GPContext.sparse_grad -- "l", "sigma", "noise", "r" (d,) and "Z" (m, d).
             With a vector l the common lengthscale is 1 and "r" is the derivative w.r.t. that vector; with a scalar l,
             "r" is the derivative w.r.t. relative lengthscales at 1.
    """
    X, Z, _ = sparse_args(X, Z, "vfe")
    l, r = split_lengthscale(l)
    ctx = ctx or default_context()
    try:
        value = ctx.sparse_fit(X, y, Z, sigma, l, noise_var, method="vfe", jitter=jitter, lengthscales=r)
        grad = ctx.sparse_grad()
    finally:
        if r is not None:
            ctx.set_lengthscales(None)                       # as every drop-in function: no lengthscales left behind
    return np.float64(value), grad
