"""Gradients of the predictive mean and variance at the test inputs, without a GPU:

1. the long-double mirror (tests/predgrad_ref.py) against central differences of its own mean and variance (h = 1e-7) for
   the four kernels, with and without lengthscales, d = 1, 3, 8 -- bar 1e-8 of the cancellation scale S;
2. the measured table: what the float64 mirror misses of the long-double mirror in that normalisation on every case the
   device is held to (tests/predgrad_cases.py), printed; the device's bars are 20 x these and never below 1e-13;
3. the mirror broken two ways (the 1 / r_k dropped from D; w replaced by v) misses its case's bar by at least 100 x;
4. the route function (gaussian_process_amd/csrc/gpmi_pgrad_plan.h) against a brute-force table, as a stand-alone program
   under g++ AddressSanitizer + UBSan (tests/sanitize/pgrad_plan_check.cpp);
5. the declaration and ctypes signature of gpmi_predict_grad_resident and gpmi_dev_back_sweep, ABI version 4, 16 timers;
6. acquisition_and_gradient against central differences of its own value for 'UCB', 'EI' and 'PI';
7. suggest_next on a NumPy stand-in context: never outside the bounds, never below its best start."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import predgrad_cases as PC
import predgrad_ref as G
from conftest import ROOT

LD = np.longdouble
H = LD(1e-7)
DIFF_BAR = 1e-8


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("d", [1, 3, 8])
def test_mirror_against_central_differences(kind, ard, d):
    """(f(x + h e_k) - f(x - h e_k)) / 2h in long double against dmu and dvar, relative to S_mu and S_var.  For nu = 1/2
    the kernel has no derivative at a training point: no test point coincides with one.  The differences themselves carry
    cond(K_y) eps_longdouble / h of noise on top of h^2: with N = 150 and noise 1e-2 (cond <= N sigma^2 / noise = 3e4)
    that is 1e-8 of var's own scale at the worst and, measured, 1e-10 of S or less."""
    N, n = 150, 4
    X, y, Xs, r = G.problem(N, d, n, seed=7 + d, lengthscales=ard, coincide=kind != "matern12")
    f = G.fit(X, y, r, kind, 1.3, PC.ell(d), 1e-2, LD)
    o = G.predict_grad(f, Xs)
    base = np.asarray(Xs, dtype=LD)
    pert = []
    for k in range(d):
        for s in (1, -1):
            P = base.copy()
            P[:, k] += s * H
            pert.append(P)
    mu, var = G.mean_var(f, np.concatenate(pert))
    mu, var = mu.reshape(d, 2, n), var.reshape(d, 2, n)
    fd_mu = ((mu[:, 0] - mu[:, 1]) / (2 * H)).T
    fd_var = ((var[:, 0] - var[:, 1]) / (2 * H)).T
    e_mu, e_var = G.err(o["dmu"], fd_mu, o["S_mu"]), G.err(o["dvar"], fd_var, o["S_var"])
    print("differences %s ard=%d d=%d: dmu %.2e dvar %.2e of the scale (bar %.0e)" % (kind, ard, d, e_mu, e_var, DIFF_BAR))
    assert e_mu <= DIFF_BAR and e_var <= DIFF_BAR


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_measured_table_of_float64(name):
    """float64 against long double on a device case: printed, finite, and far below anything a wrong formula gives"""
    c = PC.case(name)
    print("table %-24s N=%d d=%d n=%d noise=%g: float64 misses dmu %.1e dvar %.1e -> bars %.1e %.1e; max S_var/|dvar| %.1e"
          % (name, c["X"].shape[0], c["X"].shape[1], c["Xs"].shape[0], c["noise"], c["miss_mu"], c["miss_var"], c["bar_mu"],
             c["bar_var"], float(np.max(c["ld"]["S_var"] / np.abs(c["ld"]["dvar"])))))
    assert np.isfinite(c["miss_mu"]) and np.isfinite(c["miss_var"])
    assert c["bar_mu"] >= PC.FLOOR and c["bar_var"] >= PC.FLOOR
    assert c["miss_mu"] < 1e-9 and c["miss_var"] < 1e-9
    # mean and variance of the two mirrors agree as well
    assert np.allclose(np.asarray(c["f64"]["mu"]), np.asarray(c["ld"]["mu"], dtype=np.float64), rtol=0, atol=1e-7)


@pytest.mark.parametrize("name", ["rbf_d3_n37_ard_1e-4", "m32_d8_n16_ard", "m12_d3_n16_ard"])
def test_broken_mirrors_miss_the_bar(name):
    """the float64 mirror with the r_k dropped from D, and with v in the place of w: at least 100 x the case's bar"""
    c = PC.case(name)
    f = G.fit(c["X"], c["y"], c["r"], c["kind"], c["sigma"], c["l"], c["noise"])
    no_r = G.predict_grad(f, c["Xs"], broken="no_r")
    w_v = G.predict_grad(f, c["Xs"], broken="w_is_v")
    ref = c["ld"]
    e1m, e1v = G.err(no_r["dmu"], ref["dmu"], ref["S_mu"]), G.err(no_r["dvar"], ref["dvar"], ref["S_var"])
    e2v = G.err(w_v["dvar"], ref["dvar"], ref["S_var"])
    print("broken %s: no r_k dmu %.1e dvar %.1e; w = v dvar %.1e (bars %.1e %.1e)" % (name, e1m, e1v, e2v, c["bar_mu"], c["bar_var"]))
    assert e1m >= 100 * c["bar_mu"] and e1v >= 100 * c["bar_var"]
    assert e2v >= 100 * c["bar_var"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pgrad_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "pgrad_plan_check")
    subprocess.check_call([shutil.which("g++"), "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gaussian_process_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "pgrad_plan_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert "pgrad_plan_check: ok" in p.stdout


def test_predict_grad_symbols_are_additive():
    from gaussian_process_amd import _lib
    src = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+gpmi_predict_grad_resident\s*\(\s*gpmi_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*mu\s*,\s*double\s*\*\s*var\s*,"
                     r"\s*double\s*\*\s*dmu\s*,\s*double\s*\*\s*dvar\s*\)\s*;", src)
    assert re.search(r"int\s+gpmi_dev_back_sweep\s*\(\s*void\s*\*\s*stream\s*,\s*const\s+double\s*\*\s*L_dev\s*,\s*int64_t\s+ldl\s*,"
                     r"\s*int64_t\s+ncols\s*,\s*double\s*\*\s*X_dev\s*,\s*int64_t\s+ldx\s*,\s*int64_t\s+rows\s*\)\s*;", src)
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("gpmi_predict_grad_resident", 5), ("gpmi_dev_back_sweep", 7)):
        assert hasattr(raw, name), name
        assert len(_lib.SIGNATURES[name]) == nargs
    assert re.search(r"#define\s+GPMI_ABI_VERSION\s+4\b", src) and _lib.ABI_VERSION == 4
    assert re.search(r"GPMI_T_COUNT\s*=\s*16\b", src) and _lib.T_COUNT == 16
    assert raw.gpmi_abi_version() == 4


def test_python_surface_and_kernel_refusals():
    from gaussian_process_amd import GPContext
    from gaussian_process_amd import GP_regression as R
    assert callable(GPContext.predict_grad) and callable(R.suggest_next) and callable(R.acquisition_and_gradient)
    X, y = np.zeros((4, 1)), np.zeros(4)
    for kernel in ("lin", "per"):
        with pytest.raises(ValueError):
            R.prediction_gradient(X, X, y, kernel, 1.0, ctx=object())


@pytest.mark.parametrize("choice", ["UCB", "EI", "PI"])
def test_acquisitions_against_central_differences(choice):
    """mu and var as smooth functions of x: the returned gradient against differences of the returned value"""
    from gaussian_process_amd import GP_regression as R
    rng = np.random.RandomState(3)
    n, d = 9, 4
    A, B = rng.standard_normal((d,)), rng.standard_normal((d,))

    def model(Xp):
        mu = np.sin(Xp @ A) + 0.2 * (Xp ** 2).sum(1)
        var = 0.3 + 0.2 * np.cos(Xp @ B) ** 2
        dmu = np.cos(Xp @ A)[:, None] * A + 0.4 * Xp
        dvar = (-0.4 * np.cos(Xp @ B) * np.sin(Xp @ B))[:, None] * B
        return mu, var, dmu, dvar

    Xp = rng.uniform(-1, 1, size=(n, d))
    val, grad = R.acquisition_and_gradient(choice, *model(Xp), 0.4, kappa=1.7, xi=0.05)
    assert val.shape == (n,) and grad.shape == (n, d)
    h = 1e-6
    for k in range(d):
        E = np.zeros(d)
        E[k] = h
        vp, _ = R.acquisition_and_gradient(choice, *model(Xp + E), 0.4, kappa=1.7, xi=0.05)
        vm, _ = R.acquisition_and_gradient(choice, *model(Xp - E), 0.4, kappa=1.7, xi=0.05)
        fd = (vp - vm) / (2 * h)
        # central differences at h = 1e-6 of an O(1) smooth function: h^2 and 1e-16 / h, both below 1e-9
        assert np.max(np.abs(fd - grad[:, k])) <= 1e-8 * max(1.0, np.max(np.abs(grad))), (choice, k)
    with pytest.raises(ValueError):
        R.acquisition_and_gradient("XX", *model(Xp), 0.0)


class _StandIn:
    """predict_grad of a fixed smooth surrogate, as GPContext returns it; records every test set it was given"""

    def __init__(self, d):
        self.c = np.linspace(-0.5, 0.7, d)
        self.seen = []

    def predict_grad(self, Xs=None, want_var_grad=True):
        Xs = np.asarray(Xs, dtype=np.float64)
        self.seen.append(Xs.copy())
        e = Xs - self.c
        mu = np.exp(-(e ** 2).sum(1)) + 0.1 * Xs[:, 0]
        dmu = -2 * e * np.exp(-(e ** 2).sum(1))[:, None]
        dmu[:, 0] += 0.1
        var = 0.05 + 0.02 * (Xs ** 2).sum(1)
        return mu, var, dmu, 0.04 * Xs


@pytest.mark.parametrize("choice", ["UCB", "EI", "PI"])
@pytest.mark.parametrize("d", [1, 3])
def test_suggest_next_on_a_stand_in(choice, d):
    from gaussian_process_amd import GP_regression as R
    ctx = _StandIn(d)
    bounds = np.stack([np.full(d, -1.0), np.full(d, 0.5)], 1)
    x, v = R.suggest_next(bounds, choice, n_starts=16, steps=25, ctx=ctx, seed=5, y_best=0.8)
    assert x.shape == (d,) and np.all(x >= bounds[:, 0]) and np.all(x <= bounds[:, 1])
    for P in ctx.seen:                               # every step moves all starts as ONE test set, inside the box
        assert P.shape == (16, d) and np.all(P >= bounds[:, 0]) and np.all(P <= bounds[:, 1])
    start_vals, _ = R.acquisition_and_gradient(choice, *ctx.predict_grad(ctx.seen[0]), 0.8)
    assert v >= np.max(start_vals)
    again, _ = R.acquisition_and_gradient(choice, *ctx.predict_grad(x[None, :]), 0.8)
    assert again[0] == v
    assert v > np.max(start_vals) or len(ctx.seen) > 2     # it moved, or it tried to
