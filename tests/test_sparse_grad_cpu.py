"""The mirror of the VFE bound's gradient (tests/sgpr_grad_ref.py) against central differences of the bound itself
(tests/sgpr_ref.fit), both in long double, and the declaration of gpmi_sparse_grad.  No GPU.

The bar is GRAD_RTOL = 1e-8 (tests/test_parity_gpu.py) of each component's cancellation scale, the bar the device is held
to against this mirror.  The differences' own error lies far below it: h^2 = 1e-14 relative from the truncation and
eps / h = 1e-12 of the bound's scale from its rounding in long double (eps = 1.1e-19), times what an ill-conditioned K_uu
adds (cond = 1.3e7 at d = 2)."""
import os
import re

import numpy as np
import pytest

import ard_ref as R
import sgpr_grad_ref as G
import sgpr_ref as S

LD = np.longdouble
GRAD_RTOL = 1e-8
H = LD(1e-7)
SHAPES = [(130, 2, 40, 1e-2), (300, 5, 64, 5e-4), (257, 8, 130, 5e-4)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cache = {}


def _case(N, d, m, noise):
    """problem, random lengthscales and the long-double mirror: computed once, left unchanged"""
    key = (N, d, m, noise)
    if key not in _cache:
        X, y = R.problem(N, d, seed=100 + d)
        Z = S.inducing(X, m)
        r = np.random.default_rng(3).uniform(0.7, 1.6, size=d)
        _cache[key] = (X, y, Z, r, G.grad(X, y, Z, S.SIGMA, S.ELL, noise, r=r, dtype=LD))
    return _cache[key]


def _bound(X, y, Z, r, noise, sigma=S.SIGMA, l=S.ELL):
    r = np.asarray(r, dtype=LD)
    return S.fit(np.asarray(X, dtype=LD) / r, y, np.asarray(Z, dtype=LD) / r, sigma, l, noise, dtype=LD)["value"]


def _central(f, x0, h):
    return (f(LD(x0) + h) - f(LD(x0) - h)) / (2 * h)


@pytest.mark.parametrize("N,d,m,noise", SHAPES)
def test_mirror_against_central_differences(N, d, m, noise):
    X, y, Z, r, g = _case(N, d, m, noise)
    assert abs(g["value"] - _bound(X, y, Z, r, noise)) <= 1e-15 * abs(g["value"])
    errs = {}
    errs["l"] = abs(_central(lambda v: _bound(X, y, Z, r, noise, l=v), S.ELL, H) - g["g_l"]) / g["s_l"]
    errs["sigma"] = abs(_central(lambda v: _bound(X, y, Z, r, noise, sigma=v), S.SIGMA, H) - g["g_sigma"]) / g["s_sigma"]
    errs["noise"] = abs(_central(lambda v: _bound(X, y, Z, r, v), noise, H * LD(noise)) - g["g_noise"]) / g["s_noise"]
    for k in range(d):
        def f(v, k=k):
            rr = np.asarray(r, dtype=LD).copy()
            rr[k] = v
            return _bound(X, y, Z, rr, noise)
        errs["r%d" % k] = abs(_central(f, r[k], H) - g["g_r"][k]) / g["s_r"][k]
    for j, k in [(0, 0), (m // 2, d // 2), (m - 1, d - 1)]:       # first, middle, last
        def f(v, j=j, k=k):
            ZZ = np.asarray(Z, dtype=LD).copy()
            ZZ[j, k] = v
            return _bound(X, y, ZZ, r, noise)
        errs["Z%d,%d" % (j, k)] = abs(_central(f, Z[j, k], H) - g["g_Z"][j, k]) / g["s_Z"][j, k]
    print("N=%d d=%d m=%d: " % (N, d, m) + " ".join("%s %.1e" % (k, float(v)) for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= GRAD_RTOL, (k, float(v))


@pytest.mark.parametrize("N,d,m,noise", SHAPES)
def test_lengthscale_identity(N, d, m, noise):
    """sum_k r_k dF/dr_k = l dF/dl: a common factor of every r_k is a factor of l"""
    _, _, _, r, g = _case(N, d, m, noise)
    assert abs(np.sum(g["g_r"] * r) - S.ELL * g["g_l"]) <= 1e-15 * S.ELL * g["s_l"]


def test_header_and_binding_agree():
    from gaussian_process_amd import _lib
    with open(os.path.join(ROOT, "include", "gpmi.h")) as f:
        header = f.read()
    decl = re.search(r"int\s+gpmi_sparse_grad\s*\(([^)]*)\)\s*;", header)
    assert decl, "include/gpmi.h does not declare gpmi_sparse_grad"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert len(args) == 6 and args[0].startswith("gpmi_ctx*") and all(a.startswith("double*") for a in args[1:])
    assert len(_lib.SIGNATURES["gpmi_sparse_grad"]) == 6
    assert re.search(r"#define\s+GPMI_ABI_VERSION\s+4\b", header) and _lib.ABI_VERSION == 4
    assert re.search(r"GPMI_T_COUNT\s*=\s*16\b", header) and _lib.T_COUNT == 16
