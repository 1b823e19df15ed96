"""The resident-state rule (state_table.py) and the Newton step decision of the classifiers' mirrors against the one
header that holds both for the library (gaussian_process_amd/csrc/gpmi_state.h), under g++ AddressSanitizer + UBSan.
No GPU.

tests/sanitize/state_check.cpp replays event names through the header's transitions and prints what the state then
accepts; in its second mode it answers newton_decide for (psi, psi_prev, tol, halvings)."""
import os
import shutil
import subprocess

import pytest

import classify_halving as H
import state_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def state_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("state") / "state_check")
    subprocess.check_call([shutil.which("g++"), "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gaussian_process_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "state_check.cpp")])

    def ask(mode, lines, answers=None):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, mode], input="".join(q + "\n" for q in lines), env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        out = p.stdout.splitlines()
        assert len(out) == (len(lines) if answers is None else answers)
        return out
    return ask


def test_every_sequence_leaves_what_the_table_says(state_check):
    seqs = T.sequences()
    assert {ev for s in seqs for ev in s} == set(T.EVENTS)          # every event is replayed at least once
    lines = [w for s in seqs for w in ("reset",) + s]
    got = iter(state_check("events", lines, answers=sum(len(s) for s in seqs)))
    wrong = []
    for s in seqs:
        for k, want in enumerate(T.expected(s)):
            have = set(next(got).split()) - {"-"}
            if have != want:
                wrong.append("%s: after event %d table %s, header %s" % (" ".join(s), k + 1, sorted(want), sorted(have)))
    assert not wrong, "\n".join(wrong)


def test_the_table_itself():
    """a few states by hand, so that model and header cannot agree on nonsense"""
    e = T.expected(("set_train", "set_test", "factorize", "predict", "post_chol", "laplace_fit", "factorize", "predict"))
    assert e[2] == {"regression", "test"} and e[3] == {"regression", "test", "post"}
    assert e[4] == {"regression", "test", "post", T.POST_KEPT}
    assert e[5] == {"laplace", "test"} and e[6] == {"regression", "test"}
    assert e[7] == {"regression", "test", "post"}                   # the factor kept for the first v is not this v's
    e = T.expected(("set_train", "set_test", "fit_predict_sample", "predict", "set_train"))
    assert e[2] == {"regression", "test", "post", T.POST_KEPT} and e[3] == {"regression", "test", "post"} and e[4] == set()
    for a in T.FITS:
        for b in T.FITS:
            assert T.expected(("set_train", "set_test", a, b))[-1] & set(T.FIT_OF.values()) == {T.FIT_OF[b]}


def hexf(*xs):
    return " ".join(float(x).hex() for x in xs)


def test_newton_decide_takes_the_mirrors_decisions(state_check):
    """every (d, thr) of the full runs of the three step-halving problems, as psi = 0, psi_prev = -d, tol = thr (both
    exact: d = 0 - (-d), thr = tol max(1, 0)), with the number of halvings taken before it; expected is what the mirror
    did: it halved at every decision of a step but the last, and the last one either ended the run or accepted"""
    lines, want = [], []
    for kind in H.KINDS:
        ref = H.reference(kind, "full")
        assert ref["converged"]
        for k, dec in enumerate(ref["decisions"]):
            assert len(dec) == ref["halvings"][k] + 1
            for i, (d, thr) in enumerate(dec):
                lines.append(hexf(0.0, -d, thr) + " %d" % i)
                want.append("halve" if i + 1 < len(dec) else "converged" if k + 1 == len(ref["decisions"]) else "accept")
    assert {"halve", "accept", "converged"} <= set(want), set(want)
    assert want.count("halve") >= 6 and want.count("converged") == 3
    got = state_check("newton", lines)
    assert got == want, [(q, w, g) for q, w, g in zip(lines, want, got) if w != g]


def test_newton_decide_at_its_boundaries(state_check):
    up = lambda x: x * (1 + 2.0 ** -52)                 # the next float up
    cases = [
        # |d| == thr on either side is convergence, whatever the halvings; one ulp further is not
        (hexf(0.0, -0.25, 0.25) + " 0", "converged"), (hexf(0.0, 0.25, 0.25) + " 0", "converged"),
        (hexf(0.0, 0.25, 0.25) + " 20", "converged"),
        (hexf(0.0, -up(0.25), 0.25) + " 0", "accept"), (hexf(0.0, up(0.25), 0.25) + " 0", "halve"),
        # the twentieth halving is the last
        (hexf(0.0, 1.0, 0.25) + " 19", "halve"), (hexf(0.0, 1.0, 0.25) + " 20", "accept"), (hexf(0.0, 1.0, 0.25) + " 21", "accept"),
        # tol == 0: only an unchanged objective converges
        (hexf(3.5, 3.5, 0.0) + " 0", "converged"), (hexf(3.5, up(3.5), 0.0) + " 0", "halve"), (hexf(up(3.5), 3.5, 0.0) + " 0", "accept"),
        # psi == psi_prev converges for every tol
        (hexf(-7e5, -7e5, 1e-10) + " 0", "converged"), (hexf(0.0, 0.0, 0.0) + " 20", "converged"),
        # the threshold scales with |psi| above 1 and not below: thr = 2^-20 * 1024 = 2^-10, and 2^-20 for |psi| = 0.5
        (hexf(-1024.0, -1024.0 + 2.0 ** -10, 2.0 ** -20) + " 0", "converged"),
        (hexf(-1024.0, -1024.0 + 2.0 ** -9, 2.0 ** -20) + " 0", "halve"),
        (hexf(-1024.0, -1024.0 - 2.0 ** -9, 2.0 ** -20) + " 0", "accept"),
        (hexf(-0.5, -0.5 + 2.0 ** -20, 2.0 ** -20) + " 0", "converged"), (hexf(-0.5, -0.5 + 2.0 ** -19, 2.0 ** -20) + " 0", "halve"),
    ]
    got = state_check("newton", [q for q, _ in cases])
    wrong = ["%s: want %s, newton_decide %s" % (q, w, g) for (q, w), g in zip(cases, got) if g != w]
    assert not wrong, "\n".join(wrong)
