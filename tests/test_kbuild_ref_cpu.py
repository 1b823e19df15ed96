"""The exact emulation of the kernel-matrix build's two device exps (kbuild_ref.py: exp_neg_tab of rbf.hip, exp_neg_fast
of exp_dev.h) against mpmath over the directed argument set, and the exp table as the host builds it against the
correctly rounded one.  No GPU: tests/test_kbuild_routes_gpu.py holds the device to this emulation bit for bit, so the
bounds asserted here are bounds of the device."""
import numpy as np

import kbuild_ref as R


def test_directed_set_is_what_it_says():
    D = R.directed()
    n = len(D["x_core"]) + len(D["x_ext"])
    assert 12000 <= n <= 16000
    assert D["x_core"].min() >= R.NOCHECK_EDGE - 1e-9 and D["x_core"].min() < R.NOCHECK_EDGE + 1e-9
    assert D["x_ext"].max() < D["x_core"].min() and D["x_ext"].min() >= -700.0
    x = np.concatenate([D["x_core"], D["x_ext"]])
    assert 0.0 in x and -2.0 ** -53 in x
    # every table index is taken, and every binade down to the domain's end
    t = np.rint(x * R.LOG2E * R.EXP_TAB).astype(np.int64)
    assert set(t & (R.EXP_TAB - 1)) == set(range(R.EXP_TAB))
    assert set(-(t >> 12)) >= set(range(1, 1010))


def test_exp_of_minus_zero_is_one():
    for z in (0.0, -0.0):
        assert R.exp_neg_tab(z) == 1.0 and R.exp_neg_fast(z) == 1.0


def test_table_entries():
    """every entry within 0.501 ulp of 2^(j/4096); the entries that are not the correctly rounded ones are printed"""
    import mpmath
    T = R.table()
    rounded, true = R.table_true()
    assert T[0] == 1.0 and np.all(np.diff(T) > 0) and T[-1] < 2.0
    with mpmath.workprec(200):
        err = np.array([float(abs(mpmath.mpf(float(T[j])) - true[j]) * 2 ** 52) for j in range(R.EXP_TAB)])   # one ulp in [1, 2) is 2^-52
    differ = np.flatnonzero(T != rounded)
    print("table: worst entry %.6f ulp (j = %d); entries that differ from the correctly rounded table: %s"
          % (err.max(), int(err.argmax()), ", ".join("j = %d (%.6f ulp)" % (j, err[j]) for j in differ) or "none"))
    assert err.max() <= 0.501
    assert len(differ) <= 4 and np.all(np.abs(T[differ] - rounded[differ]) <= 2.0 ** -52)


def test_emulated_exps_within_their_bars():
    D = R.directed()
    for name, bar in (("tab", R.E_TAB), ("fast", R.E_FAST)):
        worst = 0.0
        for part in ("core", "ext"):
            err = R.ulp_errors(D[name + "_" + part], D["x_" + part])
            i = int(err.argmax())
            print("exp_neg_%s, %s set: worst %.4f ulp at x = %r" % (name, part, err[i], float(D["x_" + part][i])))
            worst = max(worst, err.max())
        assert worst <= bar, (name, worst)


def test_one_table_entry_moved_by_one_ulp_shows():
    """the directed set reaches every entry, so a single entry off by one ulp changes the bits of some argument"""
    D = R.directed()
    x = D["x_core"]
    j = np.rint(x * R.LOG2E * R.EXP_TAB).astype(np.int64) & (R.EXP_TAB - 1)
    x = x[j == 2069]
    assert len(x) >= 3
    T = R.table().copy()
    T[2069] = np.nextafter(T[2069], 2.0)
    assert all(R.exp_neg_tab(float(v), T) != R.exp_neg_tab(float(v)) for v in x)
