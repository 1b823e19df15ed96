"""gpmi_append without a GPU: the plan header (gaussian_process_amd/csrc/gpmi_append_plan.h) and the resident-state event
(gpmi_state.h: Resident::factor_extended) under g++ AddressSanitizer + UBSan, held against brute force by
tests/sanitize/append_plan_check.cpp; the NumPy mirror of the algorithm (tests/append_ref.py) at half the device's bar
for the factor and half the LML bar against the oracle; and the two new symbols in the header, the library and the ctypes
table with the ABI version and the timer count unchanged."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import append_ref as AR
import panel_ref as R
from conftest import ROOT

LML_RTOL = 1e-10          # tests/test_parity_gpu.py
SIGMA, ELL, NOISE = 1.0, 2.0, 1e-2


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_append_plan_and_state_under_asan_ubsan(tmp_path):
    """N around every multiple of 128 up to 1280 and around 65536, k in {1, 2, 15, 16, 17, 127, 128, 129, 1000}, with and
    without reserve: N0 and Np', the border exactly the tile rows a fresh layout of N + k adds or changes, the route, in
    place exactly when it fits, the y row moving exactly when Np' != Np; and factor_extended: the fit stays a regression,
    v, the riding posterior factor and both inverse flags go, a P-cached factor is not served for the old v, a later
    drop_fit behaves as before."""
    exe = str(tmp_path / "append_plan_check")
    subprocess.check_call([shutil.which("g++"), "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gaussian_process_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "append_plan_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert "append_plan_check: ok" in p.stdout


_problem = {}


def _case(k):
    """N = 300 points of the oracle's synthetic problem and k more; K + noise I of all of them, once per k"""
    if k not in _problem:
        import gp_oracle as O
        N = 300
        X, y, _ = O.synthetic_problem(N + k, 8, 4)
        Ky = O.RBF_kernel(X, X, SIGMA, ELL) + NOISE * np.eye(N + k)
        _problem[k] = (N, X, y, Ky)
    return _problem[k]


@pytest.mark.parametrize("k", [1, 17, 200])
def test_mirror_of_the_append(oracle, k):
    """the mirror takes the leading factor, sweeps the border rows through it with panel_ref.mirror_trsm, forms the Schur
    block, its Cholesky and m: |K_y - L L^T| <= n u |L| |L^T| componentwise (half the device's bar of 2) for the
    appended factor, and its LML within LML_RTOL / 2 of the oracle's"""
    N, X, y, Ky = _case(k)
    G, m = AR.fit(Ky[:N, :N], y[:N])
    G1, m1 = AR.append(G, m, N, Ky, y)
    N1 = N + k
    assert np.array_equal(G1[:256, :256], G[:256, :256])
    ratio = R.potrf_ratio(Ky, G1[:N1, :N1])
    fresh, mf = AR.fit(Ky, y)
    ratio_fresh = R.potrf_ratio(Ky, fresh[:N1, :N1])
    want = oracle.compute_mar_likelihood(X, None, y, SIGMA, ELL, NOISE)
    got = AR.lml(G1, m1, N1)
    print("mirror append N=300 k=%d: worst |K_y - L L^T| / (n u |L| |L^T|) = %.4f (fresh %.4f; bar 1), LML error %.2e (bar %.1e)"
          % (k, ratio, ratio_fresh, abs(got - want) / abs(want), LML_RTOL / 2))
    assert ratio <= 1, ratio
    assert abs(got - want) <= LML_RTOL / 2 * abs(want), (got, want)
    assert np.max(np.abs(m1[:N1] - mf[:N1])) <= 1e-9 / 2 * np.max(np.abs(mf[:N1]))      # half of M_RTOL


def _declared():
    src = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(gpmi_[a-z0-9_]+)\s*\(", src)), src


def test_append_symbols_are_additive():
    """gpmi_append and gpmi_dev_border_sweep are declared, exported and in the ctypes table; the ABI version stays 4 and the
    timer count 16"""
    from gaussian_process_amd import _lib
    names, src = _declared()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("gpmi_append", "gpmi_dev_border_sweep"):
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["gpmi_append"]) == 6 and len(_lib.SIGNATURES["gpmi_dev_border_sweep"]) == 7
    assert re.search(r"#define\s+GPMI_ABI_VERSION\s+4\b", src) and _lib.ABI_VERSION == 4
    assert re.search(r"GPMI_T_COUNT\s*=\s*16\b", src) and _lib.T_COUNT == 16
    assert raw.gpmi_abi_version() == 4


def test_append_python_surface():
    from gaussian_process_amd import GPContext
    from gaussian_process_amd import GP_regression as G
    assert callable(GPContext.append) and callable(G.append_observations)
