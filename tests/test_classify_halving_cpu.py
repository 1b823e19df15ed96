"""Preconditions of tests/test_classify_halving_gpu.py, on the NumPy mirrors alone, so that the GPU comparison cannot
pass vacuously: the problems of tests/classify_halving.py really halve before the iteration cap, no accept / halve
decision up to the cap sits near its threshold (a different rounding cannot flip one), and a run that never halves ends
far outside the bound the GPU is held to."""
import numpy as np
import pytest

import classify_halving as H
import laplace_ref as LR
import softmax_ref as SR


@pytest.mark.parametrize("kind", H.KINDS)
def test_the_problem_halves_before_the_cap(kind):
    ref = H.reference(kind, "capped")
    cap, first = H.CAP[kind], H.FIRST_HALVING[kind]
    assert ref["iters"] == cap and not ref["converged"]
    assert len(ref["halvings"]) == len(ref["decisions"]) == cap
    assert ref["halvings"][:first - 1] == [0] * (first - 1)
    assert ref["halvings"][first - 1] >= 1
    assert sum(ref["halvings"]) >= 2
    for n, dec in zip(ref["halvings"], ref["decisions"]):
        assert len(dec) == n + 1                       # every halving is one more decision
        assert all(d < -thr for d, thr in dec[:-1])    # ... taken because Psi fell
    full = H.reference(kind, "full")
    assert full["converged"] and full["iters"] > cap
    assert full["halvings"][:cap] == ref["halvings"]


@pytest.mark.parametrize("kind", H.KINDS)
def test_no_decision_up_to_the_cap_is_near_its_threshold(kind):
    """|d| / thr outside [1e-3, 1e3] for every decision of the capped run: a condition on the problem"""
    for dec in H.reference(kind, "capped")["decisions"]:
        for d, thr in dec:
            assert abs(d) / thr > 1e3 or abs(d) / thr < 1e-3, (d, thr)


@pytest.mark.parametrize("run", H.RUNS)
@pytest.mark.parametrize("kind", H.KINDS)
def test_a_run_without_halving_is_far_outside_the_gpu_bound(kind, run):
    """max_halvings = 0 against the halving run, in F and log q: at least 1000 times the bound of the GPU test (ten
    times the mirror's sensitivity to one rounding of K)"""
    ref = H.reference(kind, run)
    none = H.without_halving(kind, run)
    assert sum(none["halvings"]) == 0
    sens = H.sensitivity(kind, run)
    away = H.gaps(kind, none, ref)
    print(kind, run, "sensitivity", sens, "without halving", away)
    for q in ("F", "log_q"):
        assert sens[q] > 0.0
        assert away[q] >= 1000 * (10 * sens[q])


def test_two_classes_halve_where_the_binary_classifier_does():
    """the "kernel 2 K" identity holds through the halved steps: same halvings, f = F_0 - F_1"""
    b, s = H.reference("binary", "capped"), H.reference("softmax2", "capped")
    assert b["halvings"] == s["halvings"]
    assert np.max(np.abs(s["F"][0] - s["F"][1] - b["F"])) <= 1e-6 * np.max(np.abs(b["F"]))


def test_the_mirrors_default_results_are_unchanged_by_max_halvings():
    """max_halvings = 20 is the default and the records are additions: same bits with and without the argument, and a
    problem that never halves records one decision per step"""
    X, y, _ = H.data("binary")
    a = LR.laplace_fit(X[:60], y[:60], 1.0, 0.7)
    b = LR.laplace_fit(X[:60], y[:60], 1.0, 0.7, max_halvings=20)
    assert a["log_q"] == b["log_q"] and np.array_equal(a["f"], b["f"]) and a["iters"] == b["iters"]
    assert a["halvings"] == [0] * a["iters"] and [len(d) for d in a["decisions"]] == [1] * a["iters"]
    lab = H.data("softmax2")[1][:60]
    c = SR.fit(X[:60], lab, 2, 1.0, 0.7)
    d = SR.fit(X[:60], lab, 2, 1.0, 0.7, max_halvings=20)
    assert c["log_q"] == d["log_q"] and np.array_equal(c["F"], d["F"]) and c["iters"] == d["iters"]
    assert c["halvings"] == [0] * c["iters"] and [len(e) for e in c["decisions"]] == [1] * c["iters"]
