"""Host-side handle on one MI355X: NumPy in / NumPy out over the C-ABI.

`GPContext` is the object the drop-in modules (GP_regression.py,
tune_hyperparms_regression.py of this package) funnel through.  It owns a
`gpmi_ctx` (one GPU, its stream and its HBM workspaces); every array crossing
the boundary is a caller-owned float64 C-contiguous NumPy buffer.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import as_f64, check, ptr, scalar


def softmax_labels(labels, n_classes=None):
    """Host-side check of multi-class labels, before any device call: -> (labels as float64, n_classes).  Every label
    must be an integer in [0, n_classes); n_classes (default: largest label + 1) must lie in
    [2, GPMI_SOFTMAX_MAX_CLASSES]."""
    lab = as_f64(labels, 1, "labels")
    if lab.size == 0 or not np.all(np.isfinite(lab)) or np.any(lab != np.floor(lab)):
        raise ValueError("labels must be integers in [0, n_classes)")
    if n_classes is None:
        n_classes = int(lab.max()) + 1
    if n_classes != int(n_classes) or not 2 <= int(n_classes) <= _lib.SOFTMAX_MAX_CLASSES:
        raise ValueError("n_classes must be an integer in [2, %d], got %r" % (_lib.SOFTMAX_MAX_CLASSES, n_classes))
    n_classes = int(n_classes)
    if lab.min() < 0 or lab.max() >= n_classes:
        raise ValueError("labels must be integers in [0, n_classes = %d)" % n_classes)
    return lab, n_classes


def sparse_args(X, Z, method):
    """Host-side check of a sparse fit's arguments, before any device call: -> (X, Z as float64, the method's number).
    method is "vfe" or "fitc"; Z is (m, d) with the training set's d and 1 <= m <= N."""
    if method not in _lib.SPARSE_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(_lib.SPARSE_METHODS), method))
    X = as_f64(X, 2, "X_train")
    Z = as_f64(Z, 2, "Z")
    if Z.shape[1] != X.shape[1]:
        raise ValueError("Z has d=%d but the training set has d=%d" % (Z.shape[1], X.shape[1]))
    if not 1 <= Z.shape[0] <= X.shape[0]:
        raise ValueError("the number of inducing inputs must be in 1..N = %d, got %d" % (X.shape[0], Z.shape[0]))
    return X, Z, _lib.SPARSE_METHODS[method]


KEEP = object()      # lengthscales=KEEP: leave the context's per-dimension lengthscales as they are


def split_lengthscale(l):
    """A lengthscale argument of the drop-in functions -> (common l, relative lengthscales or None).  A scalar, or the
    1-element array the reference passes, is isotropic: (l, None).  A d-vector (d > 1) is one lengthscale per input
    dimension: (1.0, vector)."""
    a = np.asarray(l, dtype=np.float64)
    if a.size == 1:
        return l, None
    if a.ndim != 1:
        raise ValueError("l must be a scalar or a vector with one lengthscale per input dimension, got shape %s"
                         % (a.shape,))
    return 1.0, a


class GPContext:
    """One GPU.  Not thread-safe: use one per thread."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.gpmi_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.N = self.d = self.n = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpmi_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- options / introspection -------------------------------------------------
    def set_option(self, name, value):
        check(self._lib.gpmi_set_option(self._h, name.encode(), int(value)))

    def timers(self):
        buf = np.zeros(_lib.T_COUNT)
        check(self._lib.gpmi_get_timers(self._h, ptr(buf), _lib.T_COUNT))
        return {k: float(buf[i]) for i, k in enumerate(_lib.TIMER_NAMES)}

    def probe_mfma_f64(self):
        v = C.c_double()
        check(self._lib.gpmi_probe_mfma_f64(self._h, C.byref(v)))
        return v.value

    def probe_mfma_f64_ex(self, blocks_per_cu=2, nacc=16, iters=2048):
        """-> (TFLOP/s, shader clock GHz, cycles per MFMA per SIMD)"""
        out = np.zeros(3)
        check(self._lib.gpmi_probe_mfma_f64_ex(self._h, blocks_per_cu, nacc, iters, ptr(out)))
        return tuple(out)

    def probe_gemm(self, M, N, K, lower=0, variant=0, reps=3):
        """-> (TFLOP/s, ms per launch) of the trailing-update GEMM kernel on scratch buffers"""
        out = np.zeros(2)
        check(self._lib.gpmi_probe_gemm(self._h, M, N, K, lower, variant, reps, ptr(out)))
        return tuple(out)

    def probe_gram(self, S, m, reps=3):
        """-> (TFLOP/s, ms per call) of the sparse fit's Gram accumulation B += V^T V on a random S x m slab"""
        out = np.zeros(2)
        check(self._lib.gpmi_probe_gram(self._h, int(S), int(m), int(reps), ptr(out)))
        return tuple(out)

    def device_info(self):
        """what hipDeviceProp_t reports: CUs, clocks (kHz), memory bus width (bits), memory sizes"""
        out = np.zeros(8)
        check(self._lib.gpmi_device_info(self._h, ptr(out), 8))
        keys = ("compute_units", "clock_khz", "mem_clock_khz", "mem_bus_bits", "global_mem_bytes", "l2_bytes",
                "lds_per_workgroup_bytes", "wavefront")
        return {k: float(v) for k, v in zip(keys, out)}

    def probe_panel(self, kind, m=0, reps=20, stamps=False):
        """-> (microseconds per launch, stamps or None): potrf128 (kind 0) / trsm128 on m rows (kind 1) alone"""
        us = C.c_double()
        st = (C.c_uint64 * 64)() if stamps else None
        check(self._lib.gpmi_probe_panel(self._h, int(kind), int(m), int(reps), C.byref(us), st))
        return us.value, (np.array(st, dtype=np.uint64) if stamps else None)

    def probe_trsv_giveup(self, n=1024, wait_ms=200.0):
        """-> (err word, elapsed ms, x): the one-launch backward solve on an identity system whose bottom block is never
        solved -- every wait must run into its bound, set the error word and leave the kernel"""
        err, ms = C.c_int(-1), C.c_double()
        x = np.empty(int(n))
        check(self._lib.gpmi_probe_trsv_giveup(self._h, int(n), float(wait_ms), C.byref(err), C.byref(ms), ptr(x)))
        return err.value, ms.value, x

    def probe_hbm_write(self, nbytes=1 << 30):
        v = C.c_double()
        check(self._lib.gpmi_probe_hbm_write(self._h, int(nbytes), C.byref(v)))
        return v.value

    def probe_hbm_ex(self, nbytes, mode, blocks):
        v = C.c_double()
        check(self._lib.gpmi_probe_hbm_ex(self._h, int(nbytes), int(mode), int(blocks), C.byref(v)))
        return v.value

    # ---- a1: RBF_kernel -------------------------------------------------------------
    def rbf(self, a, b, sigma, l):
        a = as_f64(a, 2, "a")
        b = as_f64(b, 2, "b")
        if a.shape[1] != b.shape[1]:
            raise ValueError("a and b must have the same number of columns (d): %s vs %s"
                             % (a.shape, b.shape))
        out = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
        check(self._lib.gpmi_rbf(self._h, ptr(a), a.shape[0], ptr(b), b.shape[0], a.shape[1],
                                 scalar(sigma, "sigma"), scalar(l, "l"), ptr(out)))
        return out

    KINDS = {"rbf": 0, "lin": 1, "per": 2, "co2": 3, "matern12": 4, "matern32": 5, "matern52": 6}
    MATERN = {0.5: "matern12", 1.5: "matern32", 2.5: "matern52"}      # nu -> the kind's name

    def cov(self, kind, a, b, p0, p1=0.0):
        """kernel matrix of the reference's covariance functions: 'rbf' (p0 = sigma, p1 = l),
        'lin' (p0 = c), 'per' (p0 = period, p1 = lengthscale; 1-D inputs), and the Matern family 'matern12' /
        'matern32' / 'matern52' (nu = 1/2, 3/2, 5/2; p0 = sigma, p1 = l)"""
        if kind not in self.KINDS:
            raise ValueError("kind must be one of %s, got %r" % (sorted(self.KINDS), kind))
        a = as_f64(a, 2, "a")
        b = as_f64(b, 2, "b")
        if a.shape[1] != b.shape[1]:
            raise ValueError("a and b must have the same number of columns (d): %s vs %s" % (a.shape, b.shape))
        out = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
        if kind == "co2":                     # p0 = the 11 hyper-parameters (CO2_example.py:86-89)
            th = as_f64(np.asarray(p0, dtype=np.float64).reshape(-1), 1, "hyperparms")
            check(self._lib.gpmi_cov_params(self._h, 3, ptr(a), a.shape[0], ptr(b), b.shape[0], a.shape[1],
                                            ptr(th), th.shape[0], ptr(out)))
            return out
        check(self._lib.gpmi_cov(self._h, self.KINDS[kind], ptr(a), a.shape[0], ptr(b), b.shape[0], a.shape[1],
                                 scalar(p0, "p0"), scalar(p1, "p1"), ptr(out)))
        return out

    def set_kernel(self, kind, p0=0.0, p1=0.0):
        """covariance function of the following fit / predict calls (kernel_choice of prediction());
        'co2': p0 = the 11 hyper-parameters of CO2_example.py's covariance_function; 'matern12' / 'matern32' /
        'matern52' take sigma and l from the fitting call, as 'rbf' does"""
        if kind not in self.KINDS:
            raise ValueError("kind must be one of %s, got %r" % (sorted(self.KINDS), kind))
        if kind == "co2":
            th = as_f64(np.asarray(p0, dtype=np.float64).reshape(-1), 1, "hyperparms")
            check(self._lib.gpmi_set_kernel_params(self._h, 3, ptr(th), th.shape[0]))
            return
        check(self._lib.gpmi_set_kernel(self._h, self.KINDS[kind], scalar(p0, "p0"), scalar(p1, "p1")))

    # ---- fit --------------------------------------------------------------------------
    def set_train(self, X, y):
        X = as_f64(X, 2, "X_train")
        y = as_f64(y, None, "y_train").reshape(-1)
        if y.shape[0] != X.shape[0]:
            raise ValueError("X_train has %d rows but y_train has %d entries" % (X.shape[0], y.shape[0]))
        check(self._lib.gpmi_set_train(self._h, ptr(X), X.shape[0], X.shape[1], ptr(y)))
        self.N, self.d = X.shape

    def _set_train_ard(self, X, y, lengthscales):
        """set_train with the lengthscales= keyword of the fitting calls: None clears them (before the upload, so that an
        isotropic call launches what it always launched), a vector sets them for the new training set."""
        if lengthscales is None:
            self.set_lengthscales(None)
        self.set_train(X, y)
        if lengthscales is not None and lengthscales is not KEEP:
            self.set_lengthscales(lengthscales)

    def set_lengthscales(self, r):
        """Relative per-dimension lengthscales r_k > 0 (ARD): from now on this context's squared-exponential covariance
        is sigma**2 exp(-.5 / l**2 * sum_k ((x_ik - x_jk) / r_k)**2) in every fit, prediction and gradient (a Matern
        covariance takes the same scaled squared distance).  None
        returns it to the isotropic state.  Whatever was fitted is dropped; the inputs stay on the device."""
        if r is None:
            check(self._lib.gpmi_set_lengthscales(self._h, None, 0))
            return
        r = as_f64(np.asarray(r, dtype=np.float64).reshape(-1), 1, "lengthscales")
        if r.size == 0:
            raise ValueError("lengthscales must not be empty (None clears them)")
        check(self._lib.gpmi_set_lengthscales(self._h, ptr(r), r.shape[0]))

    def factorize(self, sigma, l, noise_var):
        """K + s I -> L, m = L^-1 y; returns the log-marginal-likelihood."""
        lml = C.c_double()
        bad = C.c_int64()
        st = self._lib.gpmi_factorize(self._h, scalar(sigma, "sigma"), scalar(l, "l"),
                                      scalar(noise_var, "noise_var"), C.byref(lml), C.byref(bad))
        check(st, bad.value)
        return lml.value

    def fit(self, X, y, sigma, l, noise_var, *, lengthscales=KEEP):
        self._set_train_ard(X, y, lengthscales)
        return self.factorize(sigma, l, noise_var)

    def append(self, Xnew, ynew):
        """k more observations into the resident regression fit in O(N^2 k): afterwards the context is what fit() on the
        concatenated data with the same hyper-parameters would have left.  Returns the log-marginal-likelihood of the
        N + k points; raises like factorize() when the extended matrix is not positive definite (the fit is then dropped,
        the extended training set stays).  A single point may come as a 1-D row."""
        Xnew = np.asarray(Xnew, dtype=np.float64)
        if Xnew.ndim == 1:
            Xnew = Xnew.reshape(1, -1)
        Xnew = as_f64(Xnew, 2, "X_new")
        ynew = as_f64(ynew, None, "y_new").reshape(-1)
        if ynew.shape[0] != Xnew.shape[0]:
            raise ValueError("X_new has %d rows but y_new has %d entries" % (Xnew.shape[0], ynew.shape[0]))
        if self.d and Xnew.shape[1] != self.d:
            raise ValueError("X_new has %d columns but the training set has %d" % (Xnew.shape[1], self.d))
        lml = C.c_double()
        bad = C.c_int64()
        st = self._lib.gpmi_append(self._h, ptr(Xnew), Xnew.shape[0], ptr(ynew), C.byref(lml), C.byref(bad))
        if st != _lib.GPMI_ERR_BAD_ARG:
            self.N = self.layout()["N"]        # refused: nothing changed; otherwise the context says what is resident
        check(st, bad.value)
        return lml.value

    def remove(self, idx):
        """the observations at the 0-based positions idx (distinct, any order; a single position may come as an int) out
        of the resident regression fit in O(N^2 k): afterwards the context is what fit() on the surviving points, in
        their order, with the same hyper-parameters would have left.  No element of K is evaluated, so every kernel is
        served.  Returns the log-marginal-likelihood of the surviving points."""
        idx = np.ascontiguousarray(np.asarray(idx).reshape(-1))
        if idx.size and not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("idx must hold integers, got dtype %s" % idx.dtype)
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        lml = C.c_double()
        st = self._lib.gpmi_remove(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.shape[0], C.byref(lml))
        if st != _lib.GPMI_ERR_BAD_ARG:
            self.N = self.layout()["N"]        # refused: nothing changed; otherwise the context says what is resident
        check(st)
        return lml.value

    def layout(self):
        """{N, Np, ld, rows, route} of the resident training set and factor: whether an append stayed in place shows in
        ld and rows; route is the last append's (1 skinny, 0 padded, -1 none yet)"""
        out = (C.c_int64 * 5)()
        check(self._lib.gpmi_get_layout(self._h, out))
        return dict(zip(("N", "Np", "ld", "rows", "route"), (int(v) for v in out)))

    def alpha(self):
        out = np.empty(self.N)
        check(self._lib.gpmi_get_alpha(self._h, ptr(out)))
        return out

    def m(self):
        out = np.empty(self.N)
        check(self._lib.gpmi_get_m(self._h, ptr(out)))
        return out

    def diag(self):
        out = np.empty(self.N)
        check(self._lib.gpmi_get_diag(self._h, ptr(out)))
        return out

    def factor(self, r0=0, r1=None, c0=0, c1=None):
        r1 = self.N if r1 is None else r1
        c1 = self.N if c1 is None else c1
        out = np.empty((r1 - r0, c1 - c0))
        check(self._lib.gpmi_get_factor_block(self._h, r0, r1, c0, c1, ptr(out)))
        return out

    # ---- predict ----------------------------------------------------------------------
    def set_test(self, Xs):
        Xs = as_f64(Xs, 2, "X_test")
        if Xs.shape[1] != self.d:
            raise ValueError("X_test has d=%d but the training set has d=%d" % (Xs.shape[1], self.d))
        check(self._lib.gpmi_set_test(self._h, ptr(Xs), Xs.shape[0]))
        self.n = Xs.shape[0]

    def predict_resident(self, want_sd=True):
        mu = np.empty(self.n)
        o2 = np.empty(self.n)
        check(self._lib.gpmi_predict_resident(self._h, ptr(mu), ptr(o2), 1 if want_sd else 0))
        return mu, o2

    def predict(self, Xs, want_sd=True):
        self.set_test(Xs)
        return self.predict_resident(want_sd)

    def predict_grad(self, Xs=None, want_var_grad=True):
        """Mean, variance and their gradients with respect to the test inputs at the resident regression fit:
        (mu (n,), var (n,), dmu (n, d), dvar (n, d) or None when it was not asked for).  Xs given: set_test first;
        otherwise the resident test set.  The derivatives are with respect to the raw inputs, whatever lengthscales
        are set; d sd = dvar / (2 sd) is the caller's.  Kernels 'rbf' and the Materns, d <= 32."""
        if Xs is not None:
            self.set_test(Xs)
        mu = np.empty(self.n)
        var = np.empty(self.n)
        dmu = np.empty((self.n, self.d))
        dvar = np.empty((self.n, self.d)) if want_var_grad else None
        check(self._lib.gpmi_predict_grad_resident(self._h, ptr(mu), ptr(var), ptr(dmu), ptr(dvar) if want_var_grad else None))
        return mu, var, dmu, dvar

    def fit_predict_resident(self, sigma, l, noise_var, want_sd=True):
        """prediction() in one pass (GP_regression.py:109-156) for the resident training and test sets: the rows
        K(X*, X) ride through the Cholesky below the y row.  Returns (lml, mu, sd_or_var)."""
        lml = C.c_double()
        bad = C.c_int64()
        mu = np.empty(self.n)
        o2 = np.empty(self.n)
        st = self._lib.gpmi_fit_predict_resident(self._h, scalar(sigma, "sigma"), scalar(l, "l"), scalar(noise_var, "noise_var"),
                                                 C.byref(lml), C.byref(bad), ptr(mu), ptr(o2), 1 if want_sd else 0)
        check(st, bad.value)
        return lml.value, mu, o2

    def fit_predict_sample_resident(self, sigma, l, noise_var, jitter, want_sd=True, want_factor=True):
        """prediction() with its posterior-sample factor in one pass (GP_regression.py:109-156): ONE Cholesky of
        [[K + sI, .], [K(X*, X), K_ss + jitter I]] -- L, v^T and L_ = cholesky(K_ss + jitter I - v^T v) are its blocks.
        Returns (lml, mu, sd_or_var, L_)."""
        lml = C.c_double()
        bad = C.c_int64()
        mu = np.empty(self.n)
        o2 = np.empty(self.n)
        L_ = np.empty((self.n, self.n)) if want_factor else None      # None: it stays on the device (post_sample, post_chol)
        st = self._lib.gpmi_fit_predict_sample_resident(self._h, scalar(sigma, "sigma"), scalar(l, "l"), scalar(noise_var, "noise_var"),
                                                        float(jitter), C.byref(lml), C.byref(bad), ptr(mu), ptr(o2),
                                                        1 if want_sd else 0, ptr(L_) if want_factor else None)
        check(st, bad.value)
        return lml.value, mu, o2, L_

    def fit_predict_sample(self, X, y, Xs, sigma, l, noise_var, jitter, want_sd=True, want_factor=True, *,
                           lengthscales=KEEP):
        self._set_train_ard(X, y, lengthscales)
        self.set_test(Xs)
        return self.fit_predict_sample_resident(sigma, l, noise_var, jitter, want_sd, want_factor)

    def fit_predict(self, X, y, Xs, sigma, l, noise_var, want_sd=True, *, lengthscales=KEEP):
        self._set_train_ard(X, y, lengthscales)
        self.set_test(Xs)
        return self.fit_predict_resident(sigma, l, noise_var, want_sd)

    def post_chol(self, jitter):
        out = np.empty((self.n, self.n))
        bad = C.c_int64()
        st = self._lib.gpmi_post_chol(self._h, float(jitter), ptr(out), C.byref(bad))
        check(st, bad.value)
        return out

    def post_sample(self, jitter, Z):
        """L_ @ Z with L_ = cholesky(K_ss + jitter I - v^T v) left on the device (GP_regression.py:154-155): Z (n, num_fun)
        are the caller's normals; f_post = mu[:, None] + the result."""
        Z = as_f64(Z, 2, "Z")
        if Z.shape[0] != self.n:
            raise ValueError("Z must have one row per test point: %s for n=%d" % (Z.shape, self.n))
        out = np.empty_like(Z)
        bad = C.c_int64()
        st = self._lib.gpmi_post_sample(self._h, float(jitter), ptr(Z), Z.shape[1], ptr(out), C.byref(bad))
        check(st, bad.value)
        return out

    # ---- f2: LML gradient ------------------------------------------------------------
    def lml_grad(self):
        """(dLML/dl, dLML/dsigma) at the resident factorisation:
        .5*trace((alpha alpha^T - K_y^-1) dK/dtheta) (tune_hyperparms_regression.py:43-57)."""
        dl, ds = C.c_double(), C.c_double()
        check(self._lib.gpmi_lml_grad(self._h, C.byref(dl), C.byref(ds)))
        return dl.value, ds.value

    def lml_grad_ard(self):
        """(d_r (d,), dLML/dl, dLML/dsigma, dLML/dnoise_var) at the resident factorisation: the derivatives w.r.t. the
        relative lengthscales of set_lengthscales (all 1 when none are set), the common lengthscale, the output scale
        and the noise variance, from one fused pass over K_y^-1 (gpmi_lml_grad_ard)."""
        d_r = np.empty(self.d)
        dl, ds, dn = C.c_double(), C.c_double(), C.c_double()
        check(self._lib.gpmi_lml_grad_ard(self._h, ptr(d_r), C.byref(dl), C.byref(ds), C.byref(dn)))
        return d_r, dl.value, ds.value, dn.value

    def lml_grad_co2(self):
        """(d_theta (11,), dLML/dnoise_var) at the resident factorisation of the CO2 composite kernel ('co2'): the
        derivatives w.r.t. the 11 hyper-parameters of CO2_example.py's covariance_function and the noise variance, from
        one fused pass over K_y^-1 (gpmi_lml_grad_co2)."""
        d_theta = np.empty(11)
        dn = C.c_double()
        check(self._lib.gpmi_lml_grad_co2(self._h, ptr(d_theta), C.byref(dn)))
        return d_theta, dn.value

    # ---- leave-one-out cross-validation (GPML 5.4.2) ------------------------------------
    def loo(self):
        """(mu (N,), var (N,), logp (N,), loo) at the resident regression factorisation: mean and variance of every
        training target predicted from the other N - 1 points (noise included), its log predictive probability, and
        their sum, the leave-one-out criterion of GPML eq. 5.11 (gpmi_loo)."""
        mu, var, logp = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        total = C.c_double()
        check(self._lib.gpmi_loo(self._h, ptr(mu), ptr(var), ptr(logp), C.byref(total)))
        return mu, var, logp, total.value

    def loo_grad(self):
        """(d/dl, d/dsigma, d/dnoise_var) of the leave-one-out log probability at the resident factorisation (GPML
        eq. 5.13; squared-exponential or Matern kernel, gpmi_loo_grad)."""
        dl, ds, dn = C.c_double(), C.c_double(), C.c_double()
        check(self._lib.gpmi_loo_grad(self._h, C.byref(dl), C.byref(ds), C.byref(dn)))
        return dl.value, ds.value, dn.value

    def grad_trace(self, a, b, sigma, l, alpha, K_y_inv):
        """The same two traces from gradient_ascent's arguments (tune_hyperparms_regression.py:31)."""
        a = as_f64(a, 2, "a")
        b = as_f64(b, 2, "b")
        N, d = a.shape
        if b.shape != (N, d):
            raise ValueError("a and b must both be (N, d): %s vs %s" % (a.shape, b.shape))
        al = as_f64(np.asarray(alpha, dtype=np.float64).reshape(-1), 1, "alpha")
        Ki = as_f64(K_y_inv, 2, "K_y")
        if al.shape[0] != N or Ki.shape != (N, N):
            raise ValueError("alpha must have N entries and K_y must be (N, N)")
        dl, ds = C.c_double(), C.c_double()
        check(self._lib.gpmi_grad_trace(self._h, ptr(a), ptr(b), N, d, scalar(sigma, "sigma"), scalar(l, "l"), ptr(al), ptr(Ki),
                                        C.byref(dl), C.byref(ds)))
        return dl.value, ds.value

    # ---- binary classification (Laplace approximation) --------------------------------
    def laplace_fit(self, X, y, sigma, l, *, tol=1e-10, max_iter=100, lengthscales=KEEP):
        """GPML Algorithm 3.1 (logistic likelihood) on the GPU for labels y in {-1, +1} and the squared-exponential
        kernel sigma**2 exp(-.5 sqdist / l**2).  Returns (log_q, f_hat, iters, converged): the Laplace approximation of
        the log marginal likelihood (GPML eq. 3.32), the posterior mode, the Newton steps taken and whether
        |Psi - Psi_prev| <= tol max(1, |Psi|) was reached (a RuntimeWarning when not).  The mode and the factor of
        B = I + W^1/2 K W^1/2 stay on the device for laplace_predict."""
        import warnings
        self._set_train_ard(X, y, lengthscales)
        log_q = C.c_double()
        iters, conv = C.c_int(), C.c_int()
        f_hat = np.empty(self.N)
        st = self._lib.gpmi_laplace_fit(self._h, scalar(sigma, "sigma"), scalar(l, "l"), float(tol), int(max_iter),
                                        C.byref(log_q), C.byref(iters), C.byref(conv), ptr(f_hat))
        check(st)
        if not conv.value:
            warnings.warn("Laplace approximation: Newton iteration did not converge in %d steps (tol=%g)"
                          % (iters.value, tol), RuntimeWarning, stacklevel=2)
        return log_q.value, f_hat, iters.value, bool(conv.value)

    def laplace_predict(self, Xs):
        """GPML Algorithm 3.2 on the resident Laplace fit: (f_mean, f_var, prob) of the latent function at Xs and
        prob = int expit(z) N(z | f_mean, f_var) dz, the predictive probability of the label +1."""
        self.set_test(Xs)
        f_mean, f_var, prob = np.empty(self.n), np.empty(self.n), np.empty(self.n)
        check(self._lib.gpmi_laplace_predict_resident(self._h, ptr(f_mean), ptr(f_var), ptr(prob)))
        return f_mean, f_var, prob

    def laplace_grad(self):
        """(d_r (d,), dlog_q/dl, dlog_q/dsigma) at the resident Laplace fit (GPML Algorithm 5.1): the derivatives of
        log_q w.r.t. the relative lengthscales of set_lengthscales (all 1 when none are set), the common lengthscale and
        sigma, from one fused pass over B^-1 (gpmi_laplace_grad).  The formula holds at the mode, so fit with
        tol=1e-13: the default 1e-10 leaves the fit's distance from it, up to a few 1e-9 relative, in the gradient."""
        d_r = np.empty(self.d)
        dl, ds = C.c_double(), C.c_double()
        check(self._lib.gpmi_laplace_grad(self._h, ptr(d_r), C.byref(dl), C.byref(ds)))
        return d_r, dl.value, ds.value

    # ---- multi-class classification (softmax Laplace approximation) ---------------------
    def softmax_fit(self, X, labels, n_classes, sigma, l, *, tol=1e-10, max_iter=100, lengthscales=KEEP):
        """GPML Algorithm 3.3 (softmax likelihood) on the GPU for integer labels in [0, n_classes) and one
        squared-exponential prior sigma**2 exp(-.5 sqdist / l**2) shared by the n_classes latent functions.  Returns
        (log_q, F_hat, iters, converged): the Laplace approximation of the log marginal likelihood, the posterior mode
        as an (n_classes, N) array, the Newton steps taken and whether |Psi - Psi_prev| <= tol max(1, |Psi|) was reached
        (a RuntimeWarning when not).  Y - P, the matrices E_c and the factor of sum_c E_c stay on the device for
        softmax_predict."""
        import warnings
        lab, n_classes = softmax_labels(labels, n_classes)
        self._set_train_ard(X, lab, lengthscales)
        log_q = C.c_double()
        iters, conv = C.c_int(), C.c_int()
        f_hat = np.empty((n_classes, self.N))
        st = self._lib.gpmi_softmax_fit(self._h, n_classes, scalar(sigma, "sigma"), scalar(l, "l"), float(tol),
                                        int(max_iter), C.byref(log_q), C.byref(iters), C.byref(conv), ptr(f_hat))
        check(st)
        self.n_classes = n_classes
        if not conv.value:
            warnings.warn("softmax Laplace approximation: Newton iteration did not converge in %d steps (tol=%g)"
                          % (iters.value, tol), RuntimeWarning, stacklevel=2)
        return log_q.value, f_hat, iters.value, bool(conv.value)

    def softmax_predict(self, Xs, normals=None):
        """GPML Algorithm 3.4 on the resident softmax fit: (mu, cov, prob) at Xs -- the latent mean (n, C), the latent
        covariance (n, C, C) and, when `normals` (S, C) standard normal draws are given, the class probabilities
        (n, C) = mean over s of softmax(mu + chol(cov) normals[s]) (the same draws for every test point); prob is None
        without them."""
        self.set_test(Xs)
        nc = int(getattr(self, "n_classes", 0))
        if nc < 2:
            raise ValueError("softmax_predict: no softmax fit resident (call softmax_fit)")
        mu, cov = np.empty((self.n, nc)), np.empty((self.n, nc, nc))
        S, z, prob = 0, None, None
        if normals is not None:
            z = as_f64(normals, 2, "normals")
            if z.shape[0] < 1 or z.shape[1] != nc:
                raise ValueError("normals must be (S, %d) with S >= 1, got %s" % (nc, z.shape))
            S, prob = z.shape[0], np.empty((self.n, nc))
        check(self._lib.gpmi_softmax_predict_resident(self._h, ptr(mu), ptr(cov), S, ptr(z) if S else None,
                                                      ptr(prob) if S else None))
        return mu, cov, prob

    def softmax_grad(self):
        """(d_r (d,), dlog_q/dl, dlog_q/dsigma) at the resident softmax fit: the derivatives of log_q w.r.t. the relative
        lengthscales of set_lengthscales (all 1 when none are set), the common lengthscale and sigma of the kernel the
        classes share (gpmi_softmax_grad).  The formula holds at the mode, so fit with tol=1e-13."""
        d_r = np.empty(self.d)
        dl, ds = C.c_double(), C.c_double()
        check(self._lib.gpmi_softmax_grad(self._h, ptr(d_r), C.byref(dl), C.byref(ds)))
        return d_r, dl.value, ds.value

    # ---- sparse regression with inducing points (VFE / FITC) ------------------------------
    def sparse_fit(self, X, y, Z, sigma, l, noise_var, *, method="vfe", jitter=1e-6, lengthscales=KEEP):
        """Sparse GP regression with the m inducing inputs Z (m, d), m <= N (gpmi_sparse_fit): O(N m^2) work and
        O(m^2 + N d) device memory, for N far beyond an N x N covariance.  method "vfe" returns Titsias' collapsed lower
        bound of the log marginal likelihood, "fitc" the log likelihood log N(y | 0, Q_ff + diag(K_ff - Q_ff) + noise I).
        jitter is added to the diagonal of K(Z, Z).  The factors stay on the device for sparse_predict."""
        X, Z, _ = sparse_args(X, Z, method)
        self._set_train_ard(X, y, lengthscales)
        return self.sparse_fit_resident(Z, sigma, l, noise_var, method=method, jitter=jitter)

    def sparse_fit_resident(self, Z, sigma, l, noise_var, *, method="vfe", jitter=1e-6):
        """sparse_fit on the training set and the lengthscales the context already holds (set_train, set_lengthscales):
        nothing is uploaded but Z, which is what a tuner's step wants."""
        if method not in _lib.SPARSE_METHODS:
            raise ValueError("method must be one of %s, got %r" % (sorted(_lib.SPARSE_METHODS), method))
        method_id = _lib.SPARSE_METHODS[method]
        Z = as_f64(Z, 2, "Z")
        if Z.shape[1] != self.d:
            raise ValueError("Z has d=%d but the training set has d=%d" % (Z.shape[1], self.d))
        val = C.c_double()
        bad = C.c_int64()
        st = self._lib.gpmi_sparse_fit(self._h, ptr(Z), Z.shape[0], scalar(sigma, "sigma"), scalar(l, "l"),
                                       scalar(noise_var, "noise_var"), float(jitter), method_id,
                                       C.byref(val), C.byref(bad))
        check(st, bad.value)
        self.m_inducing = Z.shape[0]
        return val.value

    def sparse_predict(self, Xs, want_sd=True):
        """(mu, sd or var) of the latent function at Xs from the resident sparse fit (gpmi_sparse_predict_resident)."""
        self.set_test(Xs)
        mu = np.empty(self.n)
        o2 = np.empty(self.n)
        check(self._lib.gpmi_sparse_predict_resident(self._h, ptr(mu), ptr(o2), 1 if want_sd else 0))
        return mu, o2

    def sparse_state(self):
        """(c (m,), q (N,)) of the resident sparse fit: c = L_B^-1 A~ y~ and q_i = |L^-1 k_u(x_i)|^2 (gpmi_sparse_get)."""
        c = np.empty(int(getattr(self, "m_inducing", 0)))
        q = np.empty(self.N)
        check(self._lib.gpmi_sparse_get(self._h, ptr(c), ptr(q)))
        return c, q

    def sparse_grad(self, want_Z=True):
        """Gradient of the VFE bound at the resident sparse fit (gpmi_sparse_grad): a dict with "l", "sigma", "noise"
        (floats), "r" (d,) -- w.r.t. the context's lengthscales, at r = 1 when it has none -- and "Z" (m, d) -- w.r.t. the
        inducing inputs as they were passed to sparse_fit; "Z" is None when want_Z is false."""
        m = int(getattr(self, "m_inducing", 0))
        dl, ds, dn = C.c_double(), C.c_double(), C.c_double()
        d_r = np.empty(self.d)
        d_Z = np.empty((m, self.d)) if want_Z else None
        check(self._lib.gpmi_sparse_grad(self._h, C.byref(dl), C.byref(ds), C.byref(dn), ptr(d_r),
                                         ptr(d_Z) if want_Z else None))
        return {"l": dl.value, "sigma": ds.value, "noise": dn.value, "r": d_r, "Z": d_Z}

    # ---- batched LML ----------------------------------------------------------------
    def lml_batch(self, triples):
        """triples: (T,3) = (l, sigma_f, noise_var) rows.  Returns (lml[T], status[T])."""
        t = as_f64(triples, 2, "triples")
        if t.shape[1] != 3:
            raise ValueError("triples must be (T, 3) = (l, sigma_f, noise_var)")
        out = np.empty(t.shape[0])
        status = np.zeros(t.shape[0], dtype=np.int32)
        check(self._lib.gpmi_lml_batch(self._h, ptr(t), t.shape[0], ptr(out),
                                       status.ctypes.data_as(C.POINTER(C.c_int))))
        return out, status


_tls = threading.local()


def default_context():
    """Per-thread lazily created context on GPMI_DEVICE (default GPU 0)."""
    import os
    ctx = getattr(_tls, "ctx", None)
    if ctx is None or ctx._h is None:
        ctx = GPContext(int(os.environ.get("GPMI_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
        _tls.ctx = ctx
    return ctx
