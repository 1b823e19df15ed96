"""Drop-in for the hot-path functions of the reference's
tune_hyperparms_regression.py (which is Python-2 syntax and cannot be imported):
`compute_mar_likelihood` (:292-313), the batch its callers loop over
(:368-369, :385-386), `bayesian_opt` (:67-101), the Bayesian-optimisation loop
(:165-289, :316-395, :418-432) and the gradient-ascent tuner (:31-64, :104-162, :398-415).
"""
from __future__ import annotations

import numpy as np

from .gp import default_context, split_lengthscale

NOISE_VAR = 0.0005      # tune_hyperparms_regression.py:302


def _use_kernel(ctx, kernel):
    """The kernel= keyword of the LML / LOO functions below: 'rbf' (the reference's, the default) or a Matern
    ('matern12', 'matern32', 'matern52').  Set on the context on every call, the way prediction() selects its kernel --
    and left there, with the factorisation the call made: a later call without the keyword sets 'rbf' again, a caller who
    goes on with the context directly finds the kernel of the last call."""
    from .GP_regression import _check_stationary
    kernel = _check_stationary(kernel)
    ctx.set_kernel(kernel)
BO_NOISE_VAR = 0.0001   # tune_hyperparms_regression.py:75


def compute_mar_likelihood(X_train, X_test, y_train, sigma, l, *, noise_var=NOISE_VAR, ctx=None, n_gpus=None,
                           dist=None, kernel="rbf"):
    """Log marginal likelihood, reference tune_hyperparms_regression.py:292-313.
    X_test is accepted and unused, exactly as in the reference.  l may be a d-vector (one lengthscale per input
    dimension); a scalar or 1-element l is isotropic and clears any the context carried.  n_gpus / dist: factorise with the covariance
    row-block partitioned over the ranks of the node (every rank makes the same call).  kernel: 'rbf' or a Matern
    ('matern12', 'matern32', 'matern52'; not on the partitioned path)."""
    from .GP_regression import _check_stationary, _dist_of
    _check_stationary(kernel)
    l, r = split_lengthscale(l)          # a d-vector: one lengthscale per input dimension, common l = 1
    gp = _dist_of(n_gpus, dist)
    if gp is not None:
        if kernel != "rbf":
            raise ValueError("the Matern kernels are not available on the partitioned path (n_gpus / dist)")
        if r is not None:
            raise ValueError("per-dimension lengthscales (a vector l) are not available on the partitioned path (n_gpus / dist)")
        from ._lib import scalar
        return np.float64(gp.fit(X_train, y_train, scalar(sigma, "sigma"), scalar(l, "l"), noise_var))
    ctx = ctx or default_context()
    _use_kernel(ctx, kernel)
    try:
        return np.float64(ctx.fit(X_train, y_train, sigma, l, noise_var, lengthscales=r))
    finally:
        if r is not None:
            ctx.set_lengthscales(None)   # the lengthscales of this call do not outlive it


def compute_mar_likelihood_batch(X_train, y_train, triples, *, ctx=None, kernel="rbf"):
    """The reference's `for i in range(len(l)): compute_mar_likelihood(...)` loops
    (:368-369, :385-386) as one call: triples is (T, 3) rows of
    (l, sigma_f, noise_var).  Returns lml (T,), NaN where K + sI was not PD.  kernel as compute_mar_likelihood."""
    ctx = ctx or default_context()
    _use_kernel(ctx, kernel)
    ctx.set_train(X_train, y_train)
    lml, _ = ctx.lml_batch(triples)
    return lml


def bayesian_opt(X_train, X_test, y_train, *, ctx=None):
    """Surrogate GP of the Bayesian-optimisation loop, reference :67-101
    (s = 1e-4, sigma = l = 1, one posterior sample)."""
    ctx = ctx or default_context()
    ctx.fit(X_train, y_train, 1, 1, BO_NOISE_VAR)          # :80-87
    mu_post, stand_devi = ctx.predict(X_test, want_sd=True)  # :90-95
    n = mu_post.shape[0]
    L_ = ctx.post_chol(1e-6)                               # :98
    f_post_fun = mu_post.reshape(-1, 1) + np.dot(L_, np.random.normal(size=(n, 1)))  # :99
    return mu_post, stand_devi, f_post_fun


# ---------------------------------------------------------------------------------------
# the Bayesian-optimisation loop around the batched LML -- a
# Python-3 restatement of tune_hyperparms_regression.py:165-289 (acquisition functions) and
# :316-395, :418-432 (candidate sampling, the loop, the driver).  Host code: the surrogate
# GP has at most ~5 points; the accelerated part is compute_mar_likelihood_batch.
# Plotting (plot_BO, the plt calls inside the acquisition functions) is out of scope.
# Pinned: the reference's own functions, print statements passed through lib2to3's fixers, were run with `random`
# and `np.random` seeded (oracle/make_golden.py:bo_loop_cases); every candidate set, surrogate posterior, chosen
# lengthscale and returned maximum of those runs is in tests/golden/kernels_bo_loops.npz, and the loops below
# reproduce them point for point (tests/test_host_logic.py on the CPU, the -m gpu tests free-running).
# ---------------------------------------------------------------------------------------
import random  # noqa: E402

from scipy.stats import norm  # noqa: E402

from .GP_regression import prediction  # noqa: E402


def _is_done(point, parms_done):
    return float(np.ravel(point)[0]) in [float(v) for v in np.ravel(parms_done)]


def PI(params, means, stand_devi, parms_done, y, n_iterations, k):
    """Probability of improvement, reference :165-204.  Returns the next point (row of
    params) or True when the early-stop criteria fire."""
    s = 0.0005
    stop_threshold = 0.001
    f_max = np.max(y) + s
    cumu_gaussian = norm.cdf((means - f_max) / stand_devi)
    if cumu_gaussian.sum() <= stop_threshold or np.max(cumu_gaussian) <= stop_threshold:
        return True                                              # :179-181
    indices = np.where(cumu_gaussian == np.max(cumu_gaussian))[0]
    next_point = params[indices[random.randint(0, len(indices) - 1)]]
    if _is_done(next_point, parms_done):                        # :189-194: one redraw, then stop
        next_point = params[indices[random.randint(0, len(indices) - 1)]]
        if _is_done(next_point, parms_done):
            return True
    return next_point


def UCB(parms_done, params, means, stand_devi, n_iterations, k):
    """Upper confidence bound, reference :207-230 (kappa = 0.001)."""
    kappa = 0.001
    objective = means + kappa * stand_devi
    next_point = params[np.where(objective == np.max(objective))[0][0]]
    if np.ravel(parms_done)[-1] == np.ravel(next_point)[0]:
        return True
    return next_point


def TS(parms_done, params, y, n_iterations, k, ctx=None):
    """Thompson sampling, reference :233-250: one posterior sample of the surrogate."""
    mu_post, stand_devi, f_post_fun = prediction(np.asarray(parms_done, dtype=np.float64).reshape(-1, 1),
                                                 params, y, 'rbf', 1, 1, ctx=ctx)
    return params[np.where(f_post_fun == np.max(f_post_fun))]


def EI(params, means, stand_devi, parms_done, y, n_iterations, k):
    """Expected improvement, reference :253-273."""
    s = 0.0005
    f_max = np.max(y) + s
    z = (means - f_max) / stand_devi
    EI_vector = (means - f_max) * norm.cdf(z) + stand_devi * norm.pdf(z)
    return params[np.where(EI_vector == np.max(EI_vector))]


def acquisition_fun(params, means, stand_devi, parms_done, y, n_iterations, k, ctx=None):
    """Reference :275-289: all four are evaluated (they consume the RNG streams in this
    order), the PI point is the one returned (:289)."""
    next_point_PI = PI(params, means, stand_devi, parms_done, y, n_iterations, k)
    UCB(parms_done, params, means, stand_devi, n_iterations, k)
    TS(parms_done, params, y, n_iterations, k, ctx=ctx)
    EI(params, means, stand_devi, parms_done, y, n_iterations, k)
    return next_point_PI


def overlap(a, b):
    """Indices of the elements of a that occur in b and where they sit in b (both unique),
    reference :316-328."""
    ind_a = np.arange(len(a))[np.isin(a, b)]
    ind_b = np.array([np.argwhere(b == a[x]) for x in ind_a]).flatten()
    return ind_a, ind_b


def random_gen_test_parms(n, parms_done):
    """n sorted candidate lengthscales from linspace(0.01, 5, n + len(done) + 10) without the
    ones already evaluated, shape (n, 1); reference :331-346."""
    num_gen = n + len(parms_done) + 10
    test_parms = np.linspace(0.01, 5, num_gen)
    _, ind_sample = overlap(np.asarray(parms_done), test_parms)
    test_parms = np.delete(test_parms, ind_sample.astype(int))
    sampled = np.asarray(random.sample(list(test_parms), n))
    return np.sort(sampled).reshape(-1, 1)


def tune_hyperparms_second(X_train, X_test, y_train, num_fun, sigma, l, *, ctx=None, verbose=False,
                           return_trace=False):
    """The BO loop, reference :349-395: 3 iterations of {LML at every lengthscale tried so
    far (one batched call here), surrogate GP, PI acquisition}; returns the best LML."""
    ctx = ctx or default_context()
    n = 100
    n_iterations = 3
    l = np.asarray(l, dtype=np.float64).reshape(-1)

    def lml_of(ls):
        triples = np.column_stack([ls, np.full(len(ls), float(sigma)), np.full(len(ls), NOISE_VAR)])
        return compute_mar_likelihood_batch(X_train, y_train, triples, ctx=ctx)

    k = 0
    for k in range(n_iterations):
        l_test = random_gen_test_parms(n, l)
        log_marg_likelihood = lml_of(l)                                          # :368-369
        mu_post, stand_devi, _ = bayesian_opt(l.reshape(-1, 1), l_test, log_marg_likelihood, ctx=ctx)   # :371
        next_point = acquisition_fun(l_test, mu_post, stand_devi, l, log_marg_likelihood, n_iterations, k,
                                     ctx=ctx)                                    # :373
        if next_point is True:                                                   # :376-380
            break
        l = np.append(l, next_point)
    log_marg_likelihood = lml_of(l)                                              # :384-386
    best = int(np.argmax(log_marg_likelihood))
    if verbose:
        print("it takes %d iterations to get the optimal!" % (k + 1))
        print("optimal lenghscalar is: %r" % l[best])
        print("maximum likelihood is: %r" % np.max(log_marg_likelihood))
    if return_trace:
        return np.max(log_marg_likelihood), l, log_marg_likelihood
    return np.max(log_marg_likelihood)


def tune_hyperparms_BO(X_train, X_test, y_train, num_fun, *, ctx=None, verbose=False):
    """Reference :418-432: sigma = 1, two random initial lengthscales in [0.02, 5)."""
    sigma = 1
    l = np.random.uniform(0.02, 5, 2)
    return tune_hyperparms_second(X_train, X_test, y_train, num_fun, sigma, l, ctx=ctx, verbose=verbose)


# ---------------------------------------------------------------------------------------
# the gradient-ascent tuner, reference :31-64, :104-162, :398-415.
# The reference inverts L twice per iteration (:144) and multiplies two N x N matrices to read
# off a trace (:55); here the inverse comes from the resident factor on the device and the
# trace is one fused pass (gpmi_lml_grad), or -- for callers that hold alpha and K_y^-1
# themselves, as gradient_ascent's signature has it -- gpmi_grad_trace.
# ---------------------------------------------------------------------------------------
GA_STEP_SIZE = 0.01      # :42
GA_TOLERANCE = 0.001     # :117
GA_MAX_ITER = 10000      # :121


def gradient_ascent(a, b, sigma, l, alpha, K_y, *, ctx=None):
    """One ascent step on the lengthscale, reference :31-64 (same arguments: alpha is
    K_y^-1 y as a column, K_y the INVERSE of K + sI).  Returns (sigma, l): sigma unchanged,
    as its update is commented out in the reference (:61)."""
    ctx = ctx or default_context()
    l_var, _ = ctx.grad_trace(a, b, sigma, l, alpha, K_y)        # :43-57
    return sigma, l + GA_STEP_SIZE * l_var                       # :63


def lml_and_gradient(X_train, y_train, sigma, l, *, noise_var=NOISE_VAR, ctx=None, kernel="rbf"):
    """LML (:141) and (dLML/dl, dLML/dsigma) (:54-57, :46-51) at (sigma, l) with everything
    resident on the device: the body of the tuner's loop without its predictive part.  kernel: 'rbf' or a Matern."""
    ctx = ctx or default_context()
    _use_kernel(ctx, kernel)
    lml = ctx.fit(X_train, y_train, sigma, l, noise_var)
    dl, ds = ctx.lml_grad()
    return np.float64(lml), dl, ds


def tune_hyperparms_first(X_train, X_test, y_train, num_fun, sigma, l, *, ctx=None, verbose=False,
                          max_iter=GA_MAX_ITER, return_trace=False):
    """Maximise the log marginal likelihood over the lengthscale by gradient ascent,
    reference :104-162.  Same constants (s = 0.0005, step 0.01, tolerance 1e-3 on |dLML|,
    at most 10000 iterations) and the same return values; the predictive mean / sd the
    reference recomputes every iteration (:131-138) are evaluated once, for the iterate the
    loop stops at -- which is what the reference returns."""
    ctx = ctx or default_context()
    ctx.set_train(X_train, y_train)
    s = NOISE_VAR                                                # :115
    log_marg_likelihood_old = 0                                  # :116
    l_eval = l
    it = 0
    for i in range(max_iter):                                    # :121
        it = i + 1
        l_eval = l
        log_marg_likelihood = np.float64(ctx.factorize(sigma, l, s))   # :123-129, :141
        l_var, _ = ctx.lml_grad()                                # :144-145 (:43-57)
        l = l + GA_STEP_SIZE * l_var                             # :63
        error = np.sqrt(np.sum((log_marg_likelihood - log_marg_likelihood_old) ** 2))   # :147
        log_marg_likelihood_old = log_marg_likelihood            # :148
        if error <= GA_TOLERANCE:                                # :149
            break
    if verbose:
        print("The hyperparameter tuning function has already converged after %d iterations!" % it)
        print("optimal lenghscalar is: %r" % float(np.asarray(l).reshape(-1)[0]))
        print("maximum log marginal likelihood is: %r" % log_marg_likelihood)
    # the factor resident now belongs to l_eval, the lengthscale of the last loop body
    mu_post, stand_devi = ctx.predict(X_test, want_sd=True)      # :131-138
    N = mu_post.shape[0]
    L_ = ctx.post_chol(1e-6)                                     # :159
    f_post_fun = mu_post.reshape(-1, 1) + np.dot(L_, np.random.normal(size=(N, num_fun)))   # :160
    if return_trace:
        return mu_post, stand_devi, f_post_fun, log_marg_likelihood, l, it
    return mu_post, stand_devi, f_post_fun, log_marg_likelihood


def tune_hyperparms_gradient(X_train, X_test, y_train, num_fun, *, ctx=None, verbose=False):
    """Reference :398-415: sigma = 1 and a random initial lengthscale in [0, 5); returns the
    maximal log marginal likelihood (the reference's plotting calls are out of scope)."""
    sigma = 1                                                    # :407
    l = np.random.uniform(0, 5, 1)                               # :408
    _, _, _, optimal_likelihood = tune_hyperparms_first(X_train, X_test, y_train, num_fun, sigma, l,
                                                        ctx=ctx, verbose=verbose)   # :410
    return optimal_likelihood


# ---------------------------------------------------------------------------------------
# Per-dimension lengthscales (ARD): the LML with its full gradient -- d lengthscales, the output scale and the noise
# variance -- from one factorisation and one fused pass over K_y^-1 (gpmi_lml_grad_ard), and a deliberately small tuner
# on top of it.  The reference has neither; anyone with an optimiser of their own calls lml_and_gradient_ard.
# ---------------------------------------------------------------------------------------
ARD_MAX_HALVINGS = 20
ARD_MAX_LOG_STEP = 1.0   # no parameter moves by more than a factor e in one trial step


def _ard_lml(ctx, lengthscales, sigma, noise_var):
    """LML at (lengthscales, sigma, noise_var) for the training set resident in ctx; -inf where K + sI is not PD."""
    ctx.set_lengthscales(lengthscales)
    try:
        return float(ctx.factorize(sigma, 1.0, noise_var))
    except np.linalg.LinAlgError:
        return -np.inf


def lml_and_gradient_ard(X_train, y_train, sigma, lengthscales, *, noise_var=NOISE_VAR, ctx=None, kernel="rbf"):
    """(lml, d_lengthscales (d,), d_sigma, d_noise): the log marginal likelihood of the squared-exponential (or, kernel=, a Matern) kernel with one
    absolute lengthscale per input dimension, and its derivatives w.r.t. those lengthscales, sigma and noise_var.  The
    context keeps the lengthscales and the factorisation (alpha, predict and lml_grad_ard work on it afterwards)."""
    ctx = ctx or default_context()
    _use_kernel(ctx, kernel)
    ls = np.asarray(lengthscales, dtype=np.float64).reshape(-1)
    lml = ctx.fit(X_train, y_train, sigma, 1.0, noise_var, lengthscales=ls)
    d_r, _, d_sigma, d_noise = ctx.lml_grad_ard()      # common l = 1: d_r is the derivative w.r.t. the lengthscales
    return np.float64(lml), d_r, d_sigma, d_noise


def _log_ascent(value, gradient, theta, max_iter, tol, n_log=None, monotone=False, gtol=None):
    """The accept / halve / step-carry ascent on the logarithms of positive parameters that tune_hyperparms_ard,
    tune_hyperparms_loo and tune_hyperparms_sparse share.  value(theta) -> the criterion at exp(theta), leaving its
    factorisation resident (-inf where K + sI is not positive definite); gradient() -> its derivatives w.r.t. exp(theta)
    at the resident point.  n_log: only the first n_log entries of theta are logarithms, the others are plain
    coordinates (the inducing inputs) whose entries of gradient() are used as they are; None: all of them.  monotone: a
    trial that is still lower after the last halving is not accepted -- the ascent stops where it stands -- so the values
    of the accepted points never decrease (without it the last trial is accepted, as the two older tuners always did).
    gtol: stop where the Euclidean norm of the gradient w.r.t. theta is at most gtol INSTEAD of where the value moved by at
    most tol max(1, |value|) (tune_hyperparms_classification: in a curved valley the halved steps move the value by less
    than that long before the gradient is small).
    -> (theta reached, its value, the values of every accepted point, the initial one first)."""
    cur = value(theta)
    if not np.isfinite(cur):
        raise np.linalg.LinAlgError("Matrix is not positive definite")
    trace = [cur]
    step = None
    for _ in range(int(max_iter)):
        jac = np.exp(theta) if n_log is None else np.concatenate([np.exp(theta[:n_log]), np.ones(theta.size - n_log)])
        g = gradient() * jac
        gmax = float(np.max(np.abs(g)))
        if not np.isfinite(gmax) or gmax == 0.0 or (gtol is not None and float(np.linalg.norm(g)) <= gtol):
            break
        cap = ARD_MAX_LOG_STEP / gmax
        step = cap if step is None else min(step, cap)
        for halving in range(ARD_MAX_HALVINGS + 1):
            trial = theta + step * g
            new = value(trial)
            if new >= cur or halving == ARD_MAX_HALVINGS:
                break
            step *= 0.5
        if not np.isfinite(new) or (monotone and new < cur):   # twenty halvings and still no factor: stay where the last one was
            value(theta)
            break
        theta = trial
        delta = abs(new - cur)
        cur = new
        trace.append(cur)
        step *= 2.0
        if gtol is None and delta <= tol * max(1.0, abs(cur)):
            break
    return theta, cur, trace


def tune_hyperparms_ard(X_train, y_train, *, sigma=1.0, lengthscales=None, noise_var=NOISE_VAR, max_iter=100, tol=1e-6,
                        ctx=None, kernel="rbf"):
    """Maximise the log marginal likelihood over (lengthscales, sigma, noise_var) by gradient ascent on their logarithms.

    Every iteration takes the gradient at the current point (d LML / d log p = p * d LML / d p) and tries a step along
    it; a step that lowers the LML (or leaves K + sI not positive definite) is halved, at most ARD_MAX_HALVINGS times,
    before being accepted -- the accept / halve rule of the classifiers' Newton loops.  The step length carries over,
    doubled, to the next iteration, and never moves a parameter by more than a factor e.  Stops after max_iter
    iterations or when |dLML| <= tol * max(1, |LML|).

    :param lengthscales: initial per-dimension lengthscales (default: all 1)
    :param kernel: 'rbf' or a Matern ('matern12', 'matern32', 'matern52'); the context keeps it
    :return: (lengthscales (d,), sigma, noise_var, lml, trace): the parameters reached, their LML and the LML of every
             accepted point, the initial one first.  The context is left with those lengthscales and their factor.
    """
    ctx = ctx or default_context()
    _use_kernel(ctx, kernel)
    X_train = np.asarray(X_train, dtype=np.float64)
    d = X_train.shape[1]
    ls = np.ones(d) if lengthscales is None else np.asarray(lengthscales, dtype=np.float64).reshape(-1).copy()
    if ls.shape[0] != d or not np.all(np.isfinite(ls)) or np.any(ls <= 0):
        raise ValueError("lengthscales must be %d finite positive numbers" % d)
    if not (sigma > 0 and noise_var > 0):
        raise ValueError("sigma and noise_var must be positive (the ascent runs on their logarithms)")
    ctx.set_train(X_train, y_train)
    theta = np.log(np.concatenate([ls, [float(sigma), float(noise_var)]]))

    def value(th):
        return _ard_lml(ctx, np.exp(th[:d]), np.exp(th[d]), np.exp(th[d + 1]))

    def gradient():
        d_r, _, d_sigma, d_noise = ctx.lml_grad_ard()
        return np.concatenate([d_r, [d_sigma, d_noise]])

    theta, lml, trace = _log_ascent(value, gradient, theta, max_iter, tol)
    return np.exp(theta[:d]), float(np.exp(theta[d])), float(np.exp(theta[d + 1])), np.float64(lml), np.asarray(trace)


# ---------------------------------------------------------------------------------------
# Leave-one-out cross-validation (GPML section 5.4.2): the second standard criterion for the hyper-parameters, more robust
# than the LML when the model is misspecified.  gpmi_loo gives the per-point held-out predictions and their log
# probability, gpmi_loo_grad its derivatives w.r.t. (l, sigma, noise_var); the reference has neither.
# ---------------------------------------------------------------------------------------
def compute_loo_likelihood(X_train, X_test, y_train, sigma, l, *, noise_var=NOISE_VAR, ctx=None, kernel="rbf"):
    """Leave-one-out log predictive probability, GPML eq. 5.11: the sibling of compute_mar_likelihood, with its argument
    handling (X_test accepted and unused; l a scalar, a 1-element array or a d-vector of per-dimension lengthscales, which
    do not outlive the call; kernel: 'rbf' or a Matern)."""
    l, r = split_lengthscale(l)
    ctx = ctx or default_context()
    _use_kernel(ctx, kernel)
    try:
        ctx.fit(X_train, y_train, sigma, l, noise_var, lengthscales=r)
        return np.float64(ctx.loo()[3])
    finally:
        if r is not None:
            ctx.set_lengthscales(None)


def loo_and_gradient(X_train, y_train, sigma, l, *, noise_var=NOISE_VAR, ctx=None, kernel="rbf"):
    """(L_LOO, dL_LOO/dl, dL_LOO/dsigma, dL_LOO/dnoise_var) at (sigma, l, noise_var) with everything resident on the
    device: the sibling of lml_and_gradient (GPML eqs. 5.11 and 5.13).  kernel: 'rbf' or a Matern."""
    ctx = ctx or default_context()
    _use_kernel(ctx, kernel)
    ctx.fit(X_train, y_train, sigma, l, noise_var)
    total = ctx.loo()[3]
    dl, ds, dn = ctx.loo_grad()
    return np.float64(total), dl, ds, dn


def tune_hyperparms_loo(X_train, y_train, *, sigma=1.0, l=1.0, noise_var=NOISE_VAR, max_iter=100, tol=1e-6, ctx=None,
                        kernel="rbf"):
    """Maximise the leave-one-out log predictive probability over (l, sigma, noise_var) by gradient ascent on their
    logarithms, with the accept / halve / step-carry rule of tune_hyperparms_ard (the same loop).  Per-dimension
    lengthscales the context carries are kept: l is then their common multiplier.

    :return: (l, sigma, noise_var, loo, trace): the parameters reached, their L_LOO and the L_LOO of every accepted point,
             the initial one first.  The context is left with the factorisation of the parameters reached.
    """
    from ._lib import scalar
    ctx = ctx or default_context()
    sigma, l, noise_var = scalar(sigma, "sigma"), scalar(l, "l"), scalar(noise_var, "noise_var")
    if not (sigma > 0 and l > 0 and noise_var > 0):
        raise ValueError("l, sigma and noise_var must be positive (the ascent runs on their logarithms)")
    _use_kernel(ctx, kernel)
    ctx.set_train(X_train, y_train)

    def value(th):
        p = np.exp(th)
        try:
            ctx.factorize(p[1], p[0], p[2])
        except np.linalg.LinAlgError:
            return -np.inf
        return float(ctx.loo()[3])

    theta, loo, trace = _log_ascent(value, lambda: np.asarray(ctx.loo_grad()), np.log([l, sigma, noise_var]), max_iter, tol)
    p = np.exp(theta)
    return float(p[0]), float(p[1]), float(p[2]), np.float64(loo), np.asarray(trace)


# ---------------------------------------------------------------------------------------
# Sparse regression: the collapsed variational bound (VFE) over the hyper-parameters and the inducing inputs, with the
# gradient of gpmi_sparse_grad.  The reference has neither.
# ---------------------------------------------------------------------------------------
def tune_hyperparms_sparse(X_train, y_train, Z, *, sigma=1.0, lengthscales=None, noise_var=NOISE_VAR, optimise_Z=True,
                           max_iter=100, tol=1e-6, jitter=1e-6, ctx=None):
    """Maximise the VFE bound of sparse GP regression over (lengthscales, sigma, noise_var) and -- optimise_Z -- the
    inducing inputs, by the ascent of tune_hyperparms_ard (the same loop): the positive parameters move on their
    logarithms, Z in its plain coordinates.  A trial point that lowers the bound, or at which K_uu + jitter I or B is
    not positive definite, halves the step; one that is still lower after the last halving ends the ascent unaccepted, so
    the bound never decreases along the trace.

    :param Z: (m, d) initial inducing inputs (choose_inducing draws a random subset)
    :param lengthscales: initial per-dimension lengthscales (default: all 1)
    :return: (lengthscales (d,), sigma, noise_var, Z (m, d), bound, trace): the parameters reached, their bound and the
             bound of every accepted point, the initial one first.  The context is left with those lengthscales and
             their sparse fit.
    """
    from .gp import sparse_args
    ctx = ctx or default_context()
    X_train, Z, _ = sparse_args(X_train, Z, "vfe")
    m, d = Z.shape
    ls = np.ones(d) if lengthscales is None else np.asarray(lengthscales, dtype=np.float64).reshape(-1).copy()
    if ls.shape[0] != d or not np.all(np.isfinite(ls)) or np.any(ls <= 0):
        raise ValueError("lengthscales must be %d finite positive numbers" % d)
    if not (sigma > 0 and noise_var > 0):
        raise ValueError("sigma and noise_var must be positive (the ascent runs on their logarithms)")
    Z0 = Z.copy()
    ctx.set_train(X_train, y_train)                 # once: every step below fits on the resident training set
    n_log = d + 2
    theta = np.concatenate([np.log(np.concatenate([ls, [float(sigma), float(noise_var)]])),
                            Z0.reshape(-1) if optimise_Z else []])

    def inducing(th):
        return np.ascontiguousarray(th[n_log:].reshape(m, d)) if optimise_Z else Z0

    def value(th):
        ctx.set_lengthscales(np.exp(th[:d]))
        try:
            return float(ctx.sparse_fit_resident(inducing(th), np.exp(th[d]), 1.0, np.exp(th[d + 1]), method="vfe",
                                                 jitter=jitter))
        except np.linalg.LinAlgError:
            return -np.inf

    def gradient():
        g = ctx.sparse_grad(want_Z=optimise_Z)      # common l = 1: "r" is the derivative w.r.t. the lengthscales
        return np.concatenate([g["r"], [g["sigma"], g["noise"]], g["Z"].reshape(-1) if optimise_Z else []])

    theta, bound, trace = _log_ascent(value, gradient, theta, max_iter, tol, n_log=n_log, monotone=True)
    return (np.exp(theta[:d]), float(np.exp(theta[d])), float(np.exp(theta[d + 1])), inducing(theta).copy(),
            np.float64(bound), np.asarray(trace))
