"""gpmi_remove without a GPU: the plan header (gaussian_process_amd/csrc/gpmi_remove_plan.h) and the resident-state event
(gpmi_state.h: Resident::factor_shrunk) under g++ AddressSanitizer + UBSan, held against brute force by
tests/sanitize/remove_plan_check.cpp; the NumPy mirror of the algorithm (tests/remove_ref.py) at half the device's bars
-- the factor's componentwise ratio against K_y of the survivors <= 1, and m, diag(L) and the LML against a fresh
factorisation of the survivors at half the bars of tests/test_append_gpu.py; and the new symbol in the header, the library
and the ctypes table with the ABI version and the timer count unchanged.

Sequences of removals are held by m, diag, alpha and the LML only: after 130 consecutive removals of index 0 from
N = 430 the plain float64 mirror's componentwise ratio is above 2 (rotations are backward stable normwise, not
componentwise), so the ratio is printed for them, not asserted."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ard_ref
import panel_ref as R
import remove_ref as RR
from conftest import ROOT

LML_RTOL, M_RTOL, ALPHA_RTOL, DIAG_RTOL = 1e-10, 1e-9, 1e-8, 1e-11      # tests/test_append_gpu.py
SIGMA, ELL, NOISE = 1.2, 1.5, 1e-2


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_remove_plan_and_state_under_asan_ubsan(tmp_path):
    """N around every multiple of 128 up to 1280 and around 65536, index sets of sizes {1, 2, 15, 16, 17, 33, 200} at the
    first index, the last index, tile edges, spread out and unsorted: the descending groups of at most 16, each sweep's
    J0, launches, N', Np', whether the y row moves, the bytes copied and streamed, the survivors' order, every refusal;
    and factor_shrunk with the effects of factor_extended."""
    exe = str(tmp_path / "remove_plan_check")
    subprocess.check_call([shutil.which("g++"), "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gaussian_process_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "remove_plan_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert "remove_plan_check: ok" in p.stdout


_problems = {}


def _problem(N, d):
    if (N, d) not in _problems:
        X, y = ard_ref.problem(N, d, seed=2000 + N + d)
        Ky = ard_ref.kernel(X, np.ones(d), SIGMA, ELL) + NOISE * np.eye(N)
        for a in (X, y, Ky):
            a.setflags(write=False)
        _problems[N, d] = (X, y, Ky)
    return _problems[N, d]


def relmax(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


def test_groups_are_descending_and_at_most_16():
    assert RR.groups([7]) == [[7]]
    assert RR.groups(range(17)) == [list(range(1, 17)), [0]]
    g = RR.groups([40, 3, 99, 5] + list(range(100, 130)))
    assert [len(x) for x in g] == [16, 16, 2] and g[-1] == [3, 5] and g[0] == list(range(114, 130))


@pytest.mark.parametrize("N,d,idx", [
    (300, 8, [137]),
    (300, 8, [5, 130, 131, 299]),
    (300, 8, [299, 5, 131, 130]),                                   # unsorted: the same result
    (300, 8, [i * 300 // 17 for i in range(17)]),                   # two sweeps
    (300, 8, list(range(0, 300, 2))),                               # ten sweeps
    (700, 8, [i * 700 // 16 + 3 for i in range(16)]),
    (600, 1, [0, 1, 2]),                                            # d = 1: cond(K_y) about 6e4
    (129, 8, [128]),
    (2, 8, [0]),
])
def test_mirror_of_the_removal(N, d, idx):
    X, y, Ky = _problem(N, d)
    G, m = RR.fit(Ky, y)
    G1, m1 = RR.remove(G, m, idx)
    keep = np.setdiff1d(np.arange(N), idx)
    Ks = Ky[np.ix_(keep, keep)]
    Gf, mf = RR.fit(Ks, y[keep])
    ratio, fresh = R.potrf_ratio(Ks, G1), R.potrf_ratio(Ks, Gf)
    e_m, e_diag = relmax(m1, mf), relmax(np.diag(G1), np.diag(Gf))
    want, got = RR.lml(Gf, mf), RR.lml(G1, m1)
    e_lml = abs(got - want) / abs(want)
    print("mirror removal N=%d d=%d k=%d: ratio %.4f (fresh %.4f; bar 1, ten sweeps 2, one survivor 4)  m %.1e  diag %.1e  lml %.1e"
          % (N, d, len(idx), ratio, fresh, e_m, e_diag, e_lml))
    assert G1.shape == (N - len(idx),) * 2 and np.all(np.triu(G1, 1) == 0) and np.all(np.diag(G1) > 0)
    j0 = min(idx)
    assert np.array_equal(G1[:j0, :j0], G[:j0, :j0]) and np.array_equal(m1[:j0], m[:j0])     # nothing in front changes
    # The bar of 1 (half the device's 2) is for what one or two sweeps do.  Two cases have a bar of their own:
    # - ten sweeps take 150 of 300 points out: every surviving element has been through up to 150 rotations, one
    #   rounding or two each, while the bound's n fell to 150 -- a sequence in all but name (module docstring); it is
    #   held to the device's own bar of 2, which the device has to meet on this very case;
    # - one survivor: the bound n u |L| |L^T| = u g^2 is below what one correctly rounded square root leaves (the fresh
    #   factor's ratio is 1.39); g = sqrt(d d + w w) is four roundings and squaring it back a fifth, each at most u / 2
    #   relative and two of them doubled by the square: 4 u.
    bar = 1 if len(idx) <= 17 and N - len(idx) > 1 else (2 if N - len(idx) > 1 else 4)
    assert ratio <= bar, (ratio, bar)
    assert e_m <= M_RTOL / 2 and e_diag <= DIAG_RTOL / 2 and e_lml <= LML_RTOL / 2
    if sorted(idx) != list(idx):
        G2, m2 = RR.remove(G, m, sorted(idx))
        assert np.array_equal(G1, G2) and np.array_equal(m1, m2)


@pytest.mark.parametrize("d", [8, 1])
def test_mirror_of_130_single_removals(d):
    """130 consecutive removals of index 0 from N = 430: m, diag(L), alpha and the LML at half the device's bars; the
    componentwise ratio of the factor is printed only (module docstring)"""
    N, steps = 430, 130
    X, y, Ky = _problem(N, d)
    G, m = RR.fit(Ky, y)
    for _ in range(steps):
        G, m = RR.remove(G, m, [0])
    Ks = Ky[steps:, steps:]
    Gf, mf = RR.fit(Ks, y[steps:])
    alpha, alpha_f = np.linalg.solve(G.T, m), np.linalg.solve(Gf.T, mf)
    e_m, e_diag, e_alpha = relmax(m, mf), relmax(np.diag(G), np.diag(Gf)), relmax(alpha, alpha_f)
    e_lml = abs(RR.lml(G, m) - RR.lml(Gf, mf)) / abs(RR.lml(Gf, mf))
    print("mirror 130 removals of index 0, d=%d: ratio %.3f (printed, not asserted)  m %.1e  diag %.1e  alpha %.1e  lml %.1e"
          % (d, R.potrf_ratio(Ks, G), e_m, e_diag, e_alpha, e_lml))
    assert e_m <= M_RTOL / 2 and e_diag <= DIAG_RTOL / 2 and e_alpha <= ALPHA_RTOL / 2 and e_lml <= LML_RTOL / 2


def _declared():
    src = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(gpmi_[a-z0-9_]+)\s*\(", src)), src


def test_remove_symbol_is_additive():
    """gpmi_remove is declared, exported and in the ctypes table; the ABI version stays 4, the timer count 16, and what
    was there before still is"""
    from gaussian_process_amd import _lib
    names, src = _declared()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("gpmi_remove", "gpmi_append", "gpmi_get_layout", "gpmi_dev_border_sweep"):
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["gpmi_remove"]) == 4 and len(_lib.SIGNATURES["gpmi_append"]) == 6
    assert re.search(r"#define\s+GPMI_ABI_VERSION\s+4\b", src) and _lib.ABI_VERSION == 4
    assert re.search(r"GPMI_T_COUNT\s*=\s*16\b", src) and _lib.T_COUNT == 16
    assert raw.gpmi_abi_version() == 4


def test_remove_python_surface():
    from gaussian_process_amd import GPContext
    from gaussian_process_amd import GP_regression as G
    assert callable(GPContext.remove) and callable(G.remove_observations) and callable(G.slide_window)
