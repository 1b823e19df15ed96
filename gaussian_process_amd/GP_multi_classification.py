"""Multi-class GP classification by the Laplace approximation on the MI355X.

Covers the compute of the reference's GP_multi_classification.py: labels are integers 0 .. C-1, every class has a latent
function with the same squared-exponential prior of RBF_kernel (kernel_parameter = sigma, l) and the likelihood is the
softmax over the C latent values.  The posterior mode is found by Newton's method and predictions average the softmax
over the Gaussian approximation, as Rasmussen & Williams, *Gaussian Processes for Machine Learning*, Algorithms 3.3 and
3.4 state them; both run on the GPU (gpmi_softmax_fit / gpmi_softmax_predict_resident of include/gpmi.h).

`softmax` and `compute_pi` keep the reference's names, arguments and returns (with `n` where the reference has the
literal 60).  Its `model_training` / `model_training2` and `prediction` are not reproduced: they build the Cn x Cn
block-diagonal kernel matrix and explicit inverses on the host, `model_training2` adds pi where the gradient has - pi,
and `prediction` returns whether one test point was labelled correctly.  `laplace_fit`, `predict_latent`, `predict_proba`
and `predict_label` below are the working forms.

`log_q_and_gradient` and `tune_hyperparms_classification` learn sigma and the lengthscales from the gradient of the
Laplace log marginal likelihood (gpmi_softmax_grad), where the reference hard-codes them.
"""
from __future__ import annotations

import numpy as np

from .gp import default_context, softmax_labels, split_lengthscale


def softmax(X):
    """exp(X) / exp(X).sum(axis=0), the softmax over the first axis (reference softmax).  The maximum is subtracted
    along that axis (the reference subtracts the global maximum, which gives the same value and underflows earlier)."""
    X = np.asarray(X, dtype=np.float64)
    e_x = np.exp(X - np.max(X, axis=0))
    return e_x / e_x.sum(axis=0)


def compute_pi(f, C, n):
    """pi_vector and pi_matrix from the stacked latent values f[c * n + i] (reference compute_pi).

    :param f: (C * n,) latent values, class-major
    :param C: number of classes
    :param n: number of training points
    :return: pi_vector (shape of f): pi_vector[c * n + i] = softmax over c of f[c * n + i];
             pi_matrix (C * n, n): column i holds the C probabilities of point i in rows i * C .. i * C + C - 1, as the
             reference fills it (GPML's Pi, the stacked diag(pi_c), would hold them in rows c * n + i)
    """
    f = np.asarray(f, dtype=np.float64)
    P = softmax(f.reshape(-1)[:C * n].reshape(C, n))
    pi_vector = P.reshape(f.shape)
    pi_matrix = np.zeros((C * n, n))
    i = np.arange(n)
    for j in range(C):
        pi_matrix[i * C + j, i] = P[j]
    return pi_vector, pi_matrix


def laplace_fit(X_train, labels, kernel_parameter=1, l=1, *, n_classes=None, ctx=None, tol=1e-10, max_iter=100):
    """Find the posterior mode of the C latent functions (GPML Algorithm 3.3) on the GPU.

    :param X_train: (N, d) inputs
    :param labels: (N,) integer labels in [0, n_classes)
    :param kernel_parameter: sigma of the RBF kernel sigma**2 exp(-.5 sqdist / l**2), shared by all classes
    :param l: lengthscale; a d-vector gives every input dimension its own (set_lengthscales(l), common l = 1) and stays
              set in ctx for the predictions; a scalar clears any the context carried
    :param n_classes: C (default: largest label + 1); 2 <= C <= 10
    :param ctx: a GPContext (default: this thread's context); the fit stays resident in it for the predictions
    :return: (log_q, F_hat, iters, converged): approximate log marginal likelihood, the mode as a (C, N) array, Newton
             steps taken, convergence flag (a RuntimeWarning is issued when False)
    """
    labels, n_classes = softmax_labels(labels, n_classes)        # refused on the host, before any device call
    ctx = default_context() if ctx is None else ctx
    l, r = split_lengthscale(l)
    return ctx.softmax_fit(X_train, labels, n_classes, kernel_parameter, l, tol=tol, max_iter=max_iter, lengthscales=r)


def predict_latent(X_test, *, ctx=None):
    """(mu, cov): latent mean (n, C) and covariance (n, C, C) at X_test from the fit resident in ctx (Algorithm 3.4)."""
    ctx = default_context() if ctx is None else ctx
    return ctx.softmax_predict(X_test)[:2]


def predict_proba(X_test, *, n_samples=1000, seed=0, normals=None, ctx=None):
    """Class probabilities (n, C): the mean of softmax(mu + chol(cov) z) over `n_samples` standard normal draws z.  The
    draws are `normals` (S, C) when given, else np.random.default_rng(seed).standard_normal((n_samples, C)); the same
    draws serve every test point, so the result is a deterministic function of the arguments."""
    ctx = default_context() if ctx is None else ctx
    if normals is None:
        nc = int(getattr(ctx, "n_classes", 0))
        if nc < 2:
            raise ValueError("predict_proba: no softmax fit resident (call laplace_fit)")
        normals = np.random.default_rng(seed).standard_normal((int(n_samples), nc))
    return ctx.softmax_predict(X_test, normals)[2]


def predict_label(X_test, *, ctx=None):
    """argmax over the classes of the latent predictive mean (the reference's `prediction`)."""
    return np.argmax(predict_latent(X_test, ctx=ctx)[0], axis=1)


# The gradient formula holds AT the mode (see GP_binary_classification.GRAD_FIT_TOL): the two functions below fit with
# 1e-13, one more Newton step at most than the default.
GRAD_FIT_TOL = 1e-13


def log_q_and_gradient(X_train, labels, sigma, lengthscales, *, n_classes=None, ctx=None, tol=GRAD_FIT_TOL, max_iter=100):
    """(log_q, d_lengthscales, d_sigma): the Laplace approximation of the log marginal likelihood of the softmax
    classifier and its derivatives w.r.t. the lengthscales and sigma of the kernel the classes share
    (gpmi_softmax_grad), the multi-class sibling of GP_binary_classification.log_q_and_gradient.

    :param lengthscales: one absolute lengthscale per input dimension -> d_lengthscales is a (d,) array; or a scalar
                         (the isotropic l, any the context carried are cleared) -> d_lengthscales is one number
    :param tol, max_iter: of the Newton iteration (see GRAD_FIT_TOL)
    The context keeps the lengthscales and the fit: predict_proba and ctx.softmax_grad() work on it afterwards.
    """
    labels, n_classes = softmax_labels(labels, n_classes)
    ctx = default_context() if ctx is None else ctx
    l, r = split_lengthscale(lengthscales)
    log_q = ctx.softmax_fit(X_train, labels, n_classes, sigma, l, tol=tol, max_iter=max_iter, lengthscales=r)[0]
    d_r, d_l, d_sigma = ctx.softmax_grad()       # a vector: common l = 1, so d_r is the derivative w.r.t. the lengthscales
    return np.float64(log_q), (np.float64(d_l) if r is None else d_r), d_sigma


def tune_hyperparms_classification(X_train, labels, *, n_classes=None, sigma=1.0, lengthscales=None, max_iter=100, tol=1e-6,
                                   ctx=None):
    """Maximise log_q over (lengthscales, sigma) by gradient ascent on their logarithms, exactly as
    GP_binary_classification.tune_hyperparms_classification does for the binary classifier: a trial that lowers log_q
    is halved and never accepted, so log_q does not decrease along the trace; the ascent stops after max_iter steps or
    where the norm of the gradient w.r.t. the logarithms is at most tol.  Every trial is a Newton fit with
    tol=GRAD_FIT_TOL.  A RuntimeWarning is issued when the ascent ends with a larger gradient norm than tol.

    :param lengthscales: initial per-dimension lengthscales (a scalar: that value for every dimension; default all 1)
    :return: (lengthscales (d,), sigma, log_q, trace): the parameters reached, their log_q and the log_q of every
             accepted point, the initial one first.  The context is left with those lengthscales and their fit, so
             predict_proba follows directly.
    """
    from .GP_binary_classification import _tune_classifier
    labels, n_classes = softmax_labels(labels, n_classes)
    ctx = default_context() if ctx is None else ctx
    return _tune_classifier(lambda sigma, ls: ctx.softmax_fit(X_train, labels, n_classes, sigma, 1.0, tol=GRAD_FIT_TOL,
                                                              lengthscales=ls)[0],
                            ctx.softmax_grad, X_train, sigma, lengthscales, max_iter, tol)
