"""Binary GP classification by the Laplace approximation on the MI355X.

Covers the compute of the reference's GP_binary_classification.py: labels are -1 / +1, the latent function has the
squared-exponential prior of RBF_kernel (kernel_parameter = sigma, l) and the likelihood is the logistic
p(y | f) = expit(y f).  The posterior mode is found by Newton's method and predictions average the logistic over the
Gaussian approximation, exactly as Rasmussen & Williams, *Gaussian Processes for Machine Learning*, Algorithms 3.1 and
3.2 state them; both run on the GPU (gpmi_laplace_fit / gpmi_laplace_predict_resident of include/gpmi.h).

The elementwise helpers keep the reference's names and semantics.  Its `model_training(K, y_train, f_prior, num_funs)`
and `prediction(...)` are not reproduced: they take and return N x N host matrices (the kernel matrix, explicit
inverses of the Cholesky factor), which is the traffic this package exists to avoid, and `model_training` evaluates
the likelihood derivatives at the prior sample `f_prior` instead of the current iterate, so W never changes and the
iteration does not find the mode; its `prediction` also drops the latent variance.  `laplace_fit`, `predict_proba` and
`predict_label` below are the working forms of those two functions.

`log_q_and_gradient` and `tune_hyperparms_classification` learn sigma and the lengthscales from the gradient of the
Laplace log marginal likelihood (GPML Algorithm 5.1, gpmi_laplace_grad), which the reference leaves to a grid search.
"""
from __future__ import annotations

import numpy as np

from .gp import default_context, split_lengthscale


def pi_function(f):
    """The logistic function expit(f) = 1 / (1 + exp(-f)) (reference pi_function)."""
    f = np.asarray(f, dtype=np.float64)
    out = np.empty_like(f)
    pos = f >= 0
    out[pos] = 1.0 / (1.0 + np.exp(-f[pos]))
    e = np.exp(f[~pos])
    out[~pos] = e / (1.0 + e)
    return out if out.ndim else float(out)


def label_function(f_star):
    """+1 where pi_function(f_star) >= 0.5 (that is, f_star >= 0), else -1 (reference label_function, elementwise)."""
    lab = np.where(np.asarray(f_star, dtype=np.float64) >= 0, 1, -1)
    return lab if lab.ndim else int(lab)


def log_likelihood(z):
    """log p(y | f) = -log(1 + exp(-z)) for z = y f (reference log_likelihood), evaluated as -softplus(-z) so that it
    does not overflow for large negative z."""
    z = np.asarray(z, dtype=np.float64)
    out = -(np.maximum(-z, 0.0) + np.log1p(np.exp(-np.abs(z))))
    return out if out.ndim else float(out)


def deriv_log_likelihood(y, f):
    """The reference's first derivative, t - pi_function(y f) with t = (y + 1) / 2.  For y = -1 this is
    -expit(-f), not the derivative -expit(f) of log p(-1 | f); the GPU fit uses GPML's t - pi_function(f)."""
    y = np.asarray(y, dtype=np.float64)
    return (y + 1) / 2 - pi_function(y * np.asarray(f, dtype=np.float64))


def sec_deriv_log_likelihood(f):
    """Second derivative of the logistic log likelihood, -pi (1 - pi) with pi = pi_function(f) (reference)."""
    p = pi_function(f)
    return -p * (1 - p)


def laplace_fit(X_train, y_train, kernel_parameter=1, l=1, *, ctx=None, tol=1e-10, max_iter=100):
    """Find the posterior mode of the latent function (GPML Algorithm 3.1) on the GPU.

    :param X_train: (N, d) inputs
    :param y_train: (N,) labels, each exactly -1 or +1
    :param kernel_parameter: sigma of the RBF kernel sigma**2 exp(-.5 sqdist / l**2)
    :param l: lengthscale; a d-vector gives every input dimension its own (set_lengthscales(l), common l = 1) and stays
              set in ctx for the predictions; a scalar clears any the context carried
    :param ctx: a GPContext (default: this thread's context); the fit stays resident in it for predict_proba
    :return: (log_q, f_hat, iters, converged): approximate log marginal likelihood (GPML eq. 3.32), the mode, Newton
             steps taken, convergence flag (a RuntimeWarning is issued when False)
    """
    ctx = default_context() if ctx is None else ctx
    l, r = split_lengthscale(l)
    return ctx.laplace_fit(X_train, y_train, kernel_parameter, l, tol=tol, max_iter=max_iter, lengthscales=r)


def predict_latent(X_test, *, ctx=None):
    """(f_mean, f_var, prob) at X_test from the fit resident in ctx (GPML Algorithm 3.2)."""
    ctx = default_context() if ctx is None else ctx
    return ctx.laplace_predict(X_test)


def predict_proba(X_test, *, ctx=None):
    """Predictive probability of the label +1, int expit(z) N(z | f_mean, f_var) dz, per test point."""
    return predict_latent(X_test, ctx=ctx)[2]


def predict_label(X_test, *, ctx=None):
    """label_function of the latent predictive mean: +1 where f_mean >= 0, else -1."""
    return label_function(predict_latent(X_test, ctx=ctx)[0])


# The gradient formula of GPML Algorithm 5.1 holds AT the mode, so whatever distance from it the Newton iteration stops
# at goes into the gradient: a few 1e-9 relative with laplace_fit's default tol=1e-10, the rounding floor (<= 1e-12) with
# 1e-13.  The two functions below therefore fit with 1e-13 (one more Newton step at most).
GRAD_FIT_TOL = 1e-13


def log_q_and_gradient(X_train, y_train, sigma, lengthscales, *, ctx=None, tol=GRAD_FIT_TOL, max_iter=100):
    """(log_q, d_lengthscales, d_sigma): the Laplace approximation of the log marginal likelihood and its derivatives
    w.r.t. the lengthscales and sigma, the classifier's sibling of lml_and_gradient_ard.

    :param lengthscales: one absolute lengthscale per input dimension -> d_lengthscales is a (d,) array; or a scalar
                         (the isotropic l, any the context carried are cleared) -> d_lengthscales is one number
    :param tol, max_iter: of the Newton iteration (see GRAD_FIT_TOL)
    The context keeps the lengthscales and the fit: predict_proba and ctx.laplace_grad() work on it afterwards.
    """
    ctx = default_context() if ctx is None else ctx
    l, r = split_lengthscale(lengthscales)
    log_q = ctx.laplace_fit(X_train, y_train, sigma, l, tol=tol, max_iter=max_iter, lengthscales=r)[0]
    d_r, d_l, d_sigma = ctx.laplace_grad()       # a vector: common l = 1, so d_r is the derivative w.r.t. the lengthscales
    return np.float64(log_q), (np.float64(d_l) if r is None else d_r), d_sigma


def tune_hyperparms_classification(X_train, y_train, *, sigma=1.0, lengthscales=None, max_iter=100, tol=1e-6, ctx=None):
    """Maximise log_q over (lengthscales, sigma) by gradient ascent on their logarithms: the loop of tune_hyperparms_ard
    with its step rule -- a trial that lowers log_q is halved, the step length carries over doubled, no parameter moves
    by more than a factor e -- in the form that never accepts a lower value, so log_q does not decrease along the trace.
    It stops after max_iter steps or where the norm of the gradient w.r.t. the logarithms is at most tol.  (Not
    tune_hyperparms_ard's |dlog_q| <= tol max(1, |log_q|): on two overlapping blobs that rule ends the ascent in a curved
    valley, where the halved steps move log_q by 1e-4 while the gradient norm is still 0.4.)  Every trial is a Newton fit
    with tol=GRAD_FIT_TOL.  A RuntimeWarning is issued when the ascent ends with a larger gradient norm than tol.

    :param lengthscales: initial per-dimension lengthscales (a scalar: that value for every dimension; default all 1)
    :return: (lengthscales (d,), sigma, log_q, trace): the parameters reached, their log_q and the log_q of every
             accepted point, the initial one first.  The context is left with those lengthscales and their fit, so
             predict_proba follows directly.
    """
    ctx = default_context() if ctx is None else ctx
    return _tune_classifier(lambda sigma, ls: ctx.laplace_fit(X_train, y_train, sigma, 1.0, tol=GRAD_FIT_TOL, lengthscales=ls)[0],
                            ctx.laplace_grad, X_train, sigma, lengthscales, max_iter, tol)


def _tune_classifier(fit, grad, X_train, sigma, lengthscales, max_iter, tol):
    """The ascent of tune_hyperparms_classification, shared with GP_multi_classification: fit(sigma, lengthscales) fits
    with common l = 1 and returns log_q, grad() returns (d_r, d_l, d_sigma) of the resident fit."""
    import warnings

    from .tune_hyperparms_regression import _log_ascent
    d = np.asarray(X_train).shape[1]
    ls = np.ones(d) if lengthscales is None else np.asarray(lengthscales, dtype=np.float64).reshape(-1).copy()
    if ls.shape[0] == 1 and d > 1:
        ls = np.full(d, ls[0])
    if ls.shape[0] != d or not np.all(np.isfinite(ls)) or np.any(ls <= 0):
        raise ValueError("lengthscales must be %d finite positive numbers" % d)
    if not sigma > 0:
        raise ValueError("sigma must be positive (the ascent runs on its logarithm)")

    def value(th):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # a trial point's unconverged fit is just a poor trial
            return float(fit(np.exp(th[d]), np.exp(th[:d])))

    def gradient():
        d_r, _, d_sigma = grad()
        return np.concatenate([d_r, [d_sigma]])

    theta, log_q, trace = _log_ascent(value, gradient, np.log(np.concatenate([ls, [float(sigma)]])), max_iter, tol,
                                      monotone=True, gtol=tol)
    gnorm = float(np.linalg.norm(gradient() * np.exp(theta)))
    if not gnorm <= tol:
        warnings.warn("tune_hyperparms_classification: stopped after %d of at most %d steps with gradient norm %.3g "
                      "(tol=%g)" % (len(trace) - 1, max_iter, gnorm, tol), RuntimeWarning, stacklevel=3)
    return np.exp(theta[:d]), float(np.exp(theta[d])), np.float64(log_q), np.asarray(trace)
