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
