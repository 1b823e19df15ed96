"""Drop-in for the hot-path functions of the reference's GP_regression.py.

Same names, positional order, return shapes/dtypes and hard-coded constants as
/root/reference/GP_regression.py (s = 0.0005 and sigma = 1 inside `prediction`,
:120-121; jitter 1e-6, :154); the arithmetic runs on the MI355X through
libgpmi355x.so.  The squared-exponential kernel is the optimised path
(BASELINE.json north_star); the reference's linear and periodic kernels
 run through the same factorisation with a plain
kernel-matrix build.
"""
from __future__ import annotations

import numpy as np

from .gp import GPContext, default_context, split_lengthscale

NOISE_VAR = 0.0005      # GP_regression.py:120
SIGMA_F = 1             # GP_regression.py:121
POST_JITTER = 1e-6      # GP_regression.py:154


def RBF_kernel(a, b, sigma, l):
    """RBF kernel matrix, reference GP_regression.py:8-19.

    :param a: (N, d) inputs
    :param b: (M, d) inputs
    :param sigma: output scale (the kernel is sigma**2 * exp(...))
    :param l: lengthscale (scalar or 1-element array), or a d-vector: one lengthscale per input dimension
    :return: (N, M) float64 covariance matrix
    """
    l, r = split_lengthscale(l)
    if r is not None:                   # both inputs scaled on the host, then the isotropic entry with l = 1
        a = np.asarray(a, dtype=np.float64) / r
        b = np.asarray(b, dtype=np.float64) / r
    return default_context().rbf(a, b, sigma, l)


def matern_kernel(a, b, sigma, l, nu=1.5):
    """Matern kernel matrix sigma**2 P(t) exp(-t), t = sqrt(2 nu) |a - b| / l, for nu = 0.5, 1.5 or 2.5 (GPML section
    4.2.1; P = 1, 1 + t, 1 + t + t**2 / 3).  The reference has none; arguments as RBF_kernel.

    :param l: lengthscale (scalar or 1-element array), or a d-vector: one lengthscale per input dimension
    :return: (N, M) float64 covariance matrix
    """
    kind = _matern_kind(nu)
    l, r = split_lengthscale(l)
    if r is not None:                   # both inputs scaled on the host, then the isotropic entry with l = 1
        a = np.asarray(a, dtype=np.float64) / r
        b = np.asarray(b, dtype=np.float64) / r
    return default_context().cov(kind, a, b, sigma, l)


def _matern_kind(nu):
    try:
        return GPContext.MATERN[float(nu)]
    except (KeyError, TypeError, ValueError):
        raise ValueError("nu must be 0.5, 1.5 or 2.5, got %r" % (nu,)) from None


STATIONARY = ('rbf', 'matern12', 'matern32', 'matern52')     # sigma and l come from the fitting call; l may be a d-vector


def _check_stationary(kernel):
    if kernel not in STATIONARY:
        raise ValueError("kernel must be one of %s, got %r" % (STATIONARY, kernel))
    return kernel


def dataset_generator(N, n):
    """Synthetic 1-D sine data, reference GP_regression.py:53-68.  Host-side and
    NumPy-RNG-order compatible (uniform then randn) so seeded runs reproduce."""
    s = 0.0005
    f = lambda x: np.sin(0.9 * x).flatten()  # noqa: E731
    X_train = np.random.uniform(-5, 5, size=(N, 1))
    y_train = f(X_train) + np.sqrt(s) * np.random.randn(N)
    X_test = np.linspace(-5, 5, n).reshape(-1, 1)
    return f, X_train, y_train, X_test


def lin_kernel(a, b, c):
    """linear kernel np.dot(a - c, b.T - c), reference GP_regression.py:22-33"""
    return default_context().cov('lin', a, b, c)


def per_kernel(a, b, parameters):
    """periodic kernel exp(-2 sin(pi |a-b| / p)^2 / l^2) on 1-D inputs, parameters = (p, l);
    reference GP_regression.py:36-50"""
    p, l = parameters
    return default_context().cov('per', a, b, p, l)


def _select_kernel(ctx, kernel_choice, parameter, sigma):
    """kernel_choice / parameter conventions of prediction() (GP_regression.py:125-136):
    'rbf': l; 'lin': the offset c; 'per': the tuple (p, l); 'matern12' / 'matern32' / 'matern52': l, as 'rbf'."""
    if kernel_choice in STATIONARY:
        ctx.set_kernel(kernel_choice)
        return sigma, parameter
    if kernel_choice == 'lin':
        ctx.set_kernel('lin', parameter)
        return 1.0, 1.0
    if kernel_choice == 'per':
        p, l = parameter
        ctx.set_kernel('per', p, l)
        return 1.0, 1.0
    raise ValueError("kernel_choice must be 'rbf', 'lin', 'per', 'matern12', 'matern32' or 'matern52', got %r"
                     % (kernel_choice,))


def _dist_of(n_gpus, dist):
    """n_gpus / dist keywords: None -> single-GPU context; a DistGP -> that; n_gpus > 1 -> the
    process-wide DistGP over WORLD (every rank must make the same call)."""
    if dist is not None:
        return dist
    if n_gpus is not None and int(n_gpus) > 1:
        from .dist import default_dist
        return default_dist(n_gpus)
    return None


def prediction(X_train, X_test, y_train, kernel_choice, l, num_fun, *, sigma=SIGMA_F,
               noise_var=NOISE_VAR, jitter=POST_JITTER, return_lml=False, ctx=None, n_gpus=None, dist=None):
    """GP posterior at the test points, reference GP_regression.py:109-156.

    With kernel_choice 'rbf' or a Matern ('matern12', 'matern32', 'matern52'), l may be a d-vector (d > 1): one lengthscale
    per input dimension.  A scalar or 1-element l
    is the reference's isotropic kernel and clears any per-dimension lengthscales the context carried.

    :return: (mu_post (n,), stand_devi (n,), f_post_fun (n, num_fun)); with return_lml=True a
             fourth element, the log marginal likelihood of the fit (tune_hyperparms_regression.py:312
             -- not the discarded expression at GP_regression.py:151, which lacks the log)
    Raises numpy.linalg.LinAlgError where the reference's np.linalg.cholesky
    would (K + sI at :138, posterior covariance at :154).  The normals of :155
    are drawn on the host from np.random in the reference's order.
    """
    r = None
    if kernel_choice in STATIONARY:
        l, r = split_lengthscale(l)     # a d-vector: one lengthscale per input dimension, common l = 1
    gp = _dist_of(n_gpus, dist)
    if gp is not None and kernel_choice in STATIONARY[1:]:
        raise ValueError("the Matern kernels are not available on the partitioned path (n_gpus / dist)")
    if gp is not None and r is not None:
        raise ValueError("per-dimension lengthscales (a vector l) are not available on the partitioned path (n_gpus / dist)")
    if gp is not None:
        # the covariance row-block partitioned over the ranks of the node (dist.py); every rank makes this call
        # with the same arguments and gets the same results; the normals of :155 come from each rank's own
        # np.random (seed them alike for identical samples)
        try:
            sg, ll = _select_kernel(gp, kernel_choice, l, sigma)      # :125-136, the same three choices on every path
            from ._lib import scalar
            lml = gp.fit(X_train, y_train, sg, scalar(ll, "l"), noise_var)
            mu_post, stand_devi = gp.predict(X_test, want_sd=True)
            L_ = gp.post_chol(jitter)
        finally:
            gp.set_kernel('rbf')
        f_post_fun = mu_post.reshape(-1, 1) + np.dot(L_, np.random.normal(size=(mu_post.shape[0], num_fun)))
        if return_lml:
            return mu_post, stand_devi, f_post_fun, np.float64(lml)
        return mu_post, stand_devi, f_post_fun
    ctx = ctx or default_context()
    try:
        sg, ll = _select_kernel(ctx, kernel_choice, l, sigma)  # :125-136
        # :126-128, 138-148 and 153-154 in one pass: ONE Cholesky of [[K + sI, .], [K(X*, X), K_ss + jitter I]] -- the test
        # rows ride through it below the training rows, and its last n columns are L_ (gpmi_fit_predict_sample_resident)
        lml, mu_post, stand_devi, _ = ctx.fit_predict_sample(X_train, y_train, X_test, sg, ll, noise_var, jitter, want_sd=True,
                                                             want_factor=False, lengthscales=r)
        n = mu_post.shape[0]
        normals = np.random.normal(size=(n, num_fun))          # :155, drawn on the host in the reference's order
        LZ = ctx.post_sample(jitter, normals)                  # L_ stays on the device: n x num_fun crosses PCIe, not n x n
    finally:
        ctx.set_kernel('rbf')
        if r is not None:
            ctx.set_lengthscales(None)  # like the kernel choice, the lengthscales of this call do not outlive it
    f_post_fun = mu_post.reshape(-1, 1) + LZ               # :155
    if return_lml:
        return mu_post, stand_devi, f_post_fun, np.float64(lml)
    return mu_post, stand_devi, f_post_fun


def append_observations(X_new, y_new, *, ctx=None):
    """Add observations to the regression fit resident in ctx (the one prediction() or ctx.fit() left) without refitting:
    O(N^2 k) instead of O(N^3).  Returns the log-marginal-likelihood of all points; predictions, gradients and
    leave-one-out calls then see the extended fit."""
    ctx = ctx or default_context()
    return ctx.append(X_new, y_new)


def remove_observations(idx, *, ctx=None):
    """Take the observations at the 0-based positions idx (distinct, any order) out of the regression fit resident in ctx
    without refitting: O(N^2 k) instead of O(N^3).  The surviving points keep their relative order.  Returns the
    log-marginal-likelihood of the surviving points; predictions, gradients, leave-one-out calls and append_observations
    then see the reduced fit."""
    ctx = ctx or default_context()
    return ctx.remove(idx)


def slide_window(X_new, y_new, *, ctx=None):
    """One step of a sliding window over a stream: the len(y_new) oldest observations leave the fit resident in ctx and
    the new ones enter it, both without refitting.  Returns the log-marginal-likelihood after the append.  With the
    context options "reserve" >= len(y_new) and "remove_keep_spare" 1 no step after the first allocates."""
    ctx = ctx or default_context()
    k = int(np.asarray(y_new).reshape(-1).shape[0])
    ctx.remove(np.arange(k))
    return ctx.append(X_new, y_new)


def f_prior(X_test, mu_prior, kernel_choice, kernel_parameter, num_fun, *, ctx=None):
    """GP prior samples, reference GP_regression.py:71-92 (s = 0.0005, sigma = 1).  With a Matern kernel_choice the
    parameter is l, a scalar or a d-vector."""
    ctx = ctx or default_context()
    X_test = np.asarray(X_test, dtype=np.float64)
    num_test = len(X_test)
    r = None
    if kernel_choice in STATIONARY[1:]:       # 'rbf' keeps the reference's scalar parameter
        kernel_parameter, r = split_lengthscale(kernel_parameter)
    try:
        sg, ll = _select_kernel(ctx, kernel_choice, kernel_parameter, SIGMA_F)      # :84-89
        if r is not None:
            ctx.fit(X_test, np.zeros(num_test), sg, ll, NOISE_VAR, lengthscales=r)
        else:
            ctx.fit(X_test, np.zeros(num_test), sg, ll, NOISE_VAR)                  # :90
        B = ctx.factor()
    finally:
        ctx.set_kernel('rbf')
        if r is not None:
            ctx.set_lengthscales(None)
    return mu_prior + np.dot(B, np.random.normal(size=(num_test, num_fun)))     # :91


def prediction_gradient(X_train, X_test, y_train, kernel_choice, l, *, sigma=SIGMA_F, noise=NOISE_VAR, ctx=None):
    """Posterior mean and variance at the test points WITH their gradients with respect to the test inputs: what a
    continuous maximisation of an acquisition function, a sensitivity analysis or input-uncertainty propagation needs
    instead of 2 d central differences per point.  Beside prediction(): same fit, kernel_choice 'rbf' or a Matern
    ('matern12', 'matern32', 'matern52'), l a scalar or a d-vector.  'lin' and 'per' raise ValueError.

    :return: (mu (n,), var (n,), dmu (n, d), dvar (n, d)); the standard deviation's gradient is dvar / (2 sqrt(var)).
    The fit stays resident in ctx WITH its kernel choice and lengthscales (suggest_next works on it); unlike prediction()
    the call does not return the context to 'rbf' -- that would drop the fit -- unless it fails."""
    _check_stationary(kernel_choice)
    l, r = split_lengthscale(l)
    ctx = ctx or default_context()
    try:
        sg, ll = _select_kernel(ctx, kernel_choice, l, sigma)
        ctx.fit(X_train, y_train, sg, ll, noise, lengthscales=r)
        return ctx.predict_grad(X_test)
    except Exception:
        ctx.set_kernel('rbf')
        if r is not None:
            ctx.set_lengthscales(None)
        raise


def _phi(u):
    return np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)


def _Phi(u):
    from math import erf
    return 0.5 * (1.0 + np.vectorize(erf, otypes=[np.float64])(u / np.sqrt(2.0)))


def acquisition_and_gradient(choice, mu, var, dmu, dvar, y_best, *, kappa=2.0, xi=0.0):
    """Value (n,) and gradient (n, d) of an acquisition function for MAXIMISATION from predict_grad's outputs (host code).
    With sd = sqrt(var), dsd = dvar / (2 sd) and u = (mu - y_best - xi) / sd:
        'UCB': mu + kappa sd                               gradient dmu + kappa dsd
        'EI':  (mu - y_best - xi) Phi(u) + sd phi(u)       gradient Phi(u) dmu + phi(u) dsd
        'PI':  Phi(u)                                      gradient phi(u) (dmu - u dsd) / sd
    y_best is not used by 'UCB'."""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    var = np.asarray(var, dtype=np.float64).reshape(-1)
    dmu = np.asarray(dmu, dtype=np.float64).reshape(mu.shape[0], -1)
    dvar = np.asarray(dvar, dtype=np.float64).reshape(mu.shape[0], -1)
    sd = np.sqrt(var)
    dsd = dvar / (2.0 * sd)[:, None]
    if choice == 'UCB':
        return mu + kappa * sd, dmu + kappa * dsd
    if choice not in ('EI', 'PI'):
        raise ValueError("choice must be 'UCB', 'EI' or 'PI', got %r" % (choice,))
    imp = mu - float(y_best) - xi
    u = imp / sd
    Phi, phi = _Phi(u), _phi(u)
    if choice == 'EI':
        return imp * Phi + sd * phi, Phi[:, None] * dmu + phi[:, None] * dsd
    return Phi, (phi / sd)[:, None] * (dmu - u[:, None] * dsd)


def suggest_next(bounds, choice='EI', *, n_starts=16, steps=50, ctx=None, seed=0, y_best=None, kappa=2.0, xi=0.0):
    """The next point to evaluate: the maximiser of an acquisition function over the box `bounds` ((d, 2): low, high) at
    the regression fit resident in ctx, by multi-start projected gradient ASCENT with backtracking.  All starts move as
    ONE test set per step (16 starts are one row group of the backward sweep), so a step is one predict_grad call plus
    one per backtracking round.  y_best (for 'EI' and 'PI'): the incumbent; None takes the largest posterior mean over
    the starting points.  Plain NumPy on the host; the starts are uniform in the box from RandomState(seed).

    :return: (x_best (d,), value): the best point found and its acquisition value -- never below the best start's."""
    ctx = ctx or default_context()
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    lo, hi = b[:, 0], b[:, 1]
    if not np.all(hi >= lo):
        raise ValueError("bounds: every high must be >= its low")
    rng = np.random.RandomState(seed)
    X = lo + (hi - lo) * rng.uniform(size=(int(n_starts), b.shape[0]))

    def evaluate(P):
        mu, var, dmu, dvar = ctx.predict_grad(P)
        return mu, var, dmu, dvar

    mu, var, dmu, dvar = evaluate(X)
    if y_best is None:
        y_best = float(np.max(mu))
    val, grad = acquisition_and_gradient(choice, mu, var, dmu, dvar, y_best, kappa=kappa, xi=xi)
    step = np.full(X.shape[0], 0.1) * float(np.max(hi - lo) if b.shape[0] else 1.0)
    for _ in range(int(steps)):
        gn = np.sqrt(np.sum(grad * grad, axis=1))
        direction = grad / np.where(gn > 0, gn, 1.0)[:, None]
        active = np.isfinite(val) & np.all(np.isfinite(grad), axis=1) & (gn > 0)
        moved = np.zeros(X.shape[0], dtype=bool)
        for _bt in range(8):                          # backtracking: halve the step of every start that did not improve
            todo = active & ~moved
            if not np.any(todo):
                break
            trial = np.clip(X + step[:, None] * direction, lo, hi)
            trial[~todo] = X[~todo]
            tmu, tvar, tdmu, tdvar = evaluate(trial)
            tval, tgrad = acquisition_and_gradient(choice, tmu, tvar, tdmu, tdvar, y_best, kappa=kappa, xi=xi)
            better = todo & np.isfinite(tval) & (tval > val)
            X[better] = trial[better]
            val[better] = tval[better]
            grad[better] = tgrad[better]
            moved |= better
            step[todo & ~better] *= 0.5
        step[moved] *= 1.5
        if not np.any(moved):
            break
    best = int(np.nanargmax(val))
    return X[best].copy(), float(val[best])
