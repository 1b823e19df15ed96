"""Leave-one-out cross-validation without a GPU: the NumPy mirror of tests/loo_ref.py checked against itself -- its closed
forms against N brute-force fits with one point deleted, its three derivatives against central differences of its own
total -- and the C-ABI's declarations of the two calls."""
import os
import re

import numpy as np
import pytest

import ard_ref as R
import loo_ref as LR
from conftest import ROOT

LML_RTOL = 1e-10      # tests/test_parity_gpu.py
SIGMA, ELL = 1.2, 1.3
# (130, 2) at noise 5e-4 has a condition number of 1.5e5 and is left out on purpose
CASES = [(130, 2, 1e-2), (300, 5, 5e-4), (257, 8, 5e-4)]


def _problem(N, d):
    return R.problem(N, d, seed=100 + d)


@pytest.mark.parametrize("N,d,noise", CASES)
def test_closed_forms_against_brute_force(N, d, noise):
    X, y = _problem(N, d)
    r = np.ones(d)
    a = LR.values(X, y, r, SIGMA, ELL, noise)
    b = LR.brute(X, y, r, SIGMA, ELL, noise)
    e_mu = np.max(np.abs(a["mu"] - b["mu"]))
    e_var = np.max(np.abs(a["var"] - b["var"]) / b["var"])
    e_tot = abs(a["loo"] - b["loo"]) / abs(b["loo"])
    print("N=%d d=%d noise=%g cond %.2e: mu %.2e var %.2e total %.2e" % (N, d, noise, a["cond"], e_mu, e_var, e_tot))
    assert e_mu <= 1e-10
    assert e_var <= 1e-10
    assert e_tot <= LML_RTOL


@pytest.mark.parametrize("N,d,noise", CASES)
def test_derivatives_against_central_differences(N, d, noise):
    X, y = _problem(N, d)
    r = np.ones(d)
    ref = LR.closed(X, y, r, SIGMA, ELL, noise)
    theta = {"l": ELL, "sigma": SIGMA, "noise": noise}

    def f(**kw):
        p = dict(theta, **kw)
        return LR.total(X, y, r, p["sigma"], p["l"], p["noise"])

    for name in ("l", "sigma", "noise"):
        h = 1e-5 * theta[name]
        fd = (f(**{name: theta[name] + h}) - f(**{name: theta[name] - h})) / (2 * h)
        err = abs(fd - ref["g_" + name]) / ref["s_" + name]
        print("N=%d d=%d %s: closed %.9e differences %.9e, error / scale %.2e" % (N, d, name, ref["g_" + name], fd, err))
        assert err <= 1e-6, (name, fd, ref["g_" + name], ref["s_" + name])


def test_header_declares_and_the_shim_binds_both_calls():
    src = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+gpmi_loo\s*\(\s*gpmi_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*mu\s*,\s*double\s*\*\s*var\s*,"
                     r"\s*double\s*\*\s*logp\s*,\s*double\s*\*\s*loo\s*\)\s*;", code)
    assert re.search(r"\bint\s+gpmi_loo_grad\s*\(\s*gpmi_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*d_ell\s*,\s*double\s*\*\s*d_sigma\s*,"
                     r"\s*double\s*\*\s*d_noise\s*\)\s*;", code)
    assert re.search(r"\bGPMI_T_LOO\s*=\s*13\b", code)
    assert re.search(r"\bGPMI_T_COUNT\s*=\s*16\b", code) and re.search(r"#define\s+GPMI_ABI_VERSION\s+4\b", code)
    from gaussian_process_amd import _lib
    assert len(_lib.SIGNATURES["gpmi_loo"]) == 5 and len(_lib.SIGNATURES["gpmi_loo_grad"]) == 4
    assert _lib.TIMER_NAMES[13] == "loo" and _lib.ABI_VERSION == 4
