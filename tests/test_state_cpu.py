"""The resident-state rule (state_table.py), the Newton step decision and the Newton loop of the classifiers' mirrors
against the one header that holds all three for the library (gaussian_process_amd/csrc/gpmi_state.h), under g++
AddressSanitizer + UBSan.  No GPU.

tests/sanitize/state_check.cpp replays event names through the header's transitions and prints what the state then
accepts; in its second mode it answers newton_decide for (psi, psi_prev, tol, halvings); in its third it runs
newton_iterate on a scripted objective and prints the calls the loop made."""
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


def run_line(tol, max_iter, psis, fail="-", nth=0, status=0):
    return "%s %d %s %d %d %s" % (hexf(tol), max_iter, fail, nth, status, hexf(*psis))


TOL = 2.0 ** -10         # of the scripted runs: the threshold tol max(1, |Psi|) stays under 1 for every |Psi| below 1024


def parse_run(line):
    """-> (trace words, iters, converged, status)"""
    words = line.split()
    return words[:-3], int(words[-3]), int(words[-2]), int(words[-1])


def test_newton_iterate_by_hand(state_check):
    halve20 = ["forward", "eval0"] + ["eval1"] * 20 + ["factor0", "step"]
    cases = [
        # max_iter = 0: one evaluation, the factor of the start, nothing else
        (run_line(TOL, 0, [3.0]), ("forward eval0 factor1".split(), 0, 0, 0)),
        # the first comparison (there is none before the first step) converges: the last factor, no step behind it
        (run_line(TOL, 5, [-10.0, -10.0 - 2.0 ** -7]), ("forward eval0 factor0 step forward eval0 factor1".split(), 1, 1, 0)),
        # the cap: rising all the way, max_iter steps and the factor of iterate max_iter
        (run_line(TOL, 2, [-10.0, -5.0, -2.0]),
         ("forward eval0 factor0 step forward eval0 factor0 step forward eval0 factor1".split(), 2, 0, 0)),
        # ... and converging exactly at the cap counts as converged
        (run_line(TOL, 1, [-10.0, -10.0]), ("forward eval0 factor0 step forward eval0 factor1".split(), 1, 1, 0)),
        # one halving: the halved step's Psi is the one the next comparison is made against (-8 -> -8 - 2^-8 converges,
        # which it would not against -20 or -10)
        (run_line(TOL, 9, [-10.0, -20.0, -8.0, -8.0 - 2.0 ** -8]),
         ("forward eval0 factor0 step forward eval0 eval1 factor0 step forward eval0 factor1".split(), 2, 1, 0)),
        # twenty halvings of a step that keeps falling, then it is accepted as it is
        (run_line(TOL, 9, [0.0] + [-10.0 - k for k in range(21)] + [-30.0]),
         ("forward eval0 factor0 step".split() + halve20 + "forward eval0 factor1".split(), 2, 1, 0)),
        # a status from each callback ends the run there, with that status and nothing reported
        (run_line(TOL, 9, [0.0, 5.0], "forward", 1, 7), (["forward"], -1, -1, 7)),
        (run_line(TOL, 9, [0.0, 5.0], "forward", 2, 7), ("forward eval0 factor0 step forward".split(), -1, -1, 7)),
        (run_line(TOL, 9, [0.0, 5.0], "eval", 1, 3), ("forward eval0".split(), -1, -1, 3)),
        (run_line(TOL, 9, [0.0, -5.0, -4.0], "eval", 3, 3), ("forward eval0 factor0 step forward eval0 eval1".split(), -1, -1, 3)),
        (run_line(TOL, 9, [0.0, 5.0], "factor", 1, 2), ("forward eval0 factor0".split(), -1, -1, 2)),
        (run_line(TOL, 0, [0.0], "factor", 1, 2), ("forward eval0 factor1".split(), -1, -1, 2)),
        (run_line(TOL, 9, [0.0, 5.0], "step", 1, 1), ("forward eval0 factor0 step".split(), -1, -1, 1)),
        (run_line(TOL, 9, [0.0, 5.0, 9.0], "step", 2, -4),
         ("forward eval0 factor0 step forward eval0 factor0 step".split(), -1, -1, -4)),
    ]
    got = [parse_run(g) for g in state_check("iterate", [q for q, _ in cases])]
    wrong = ["%s: want %s, newton_iterate %s" % (q, w, g) for (q, w), g in zip(cases, got) if g != w]
    assert not wrong, "\n".join(wrong)


def test_newton_iterate_takes_the_mirrors_runs(state_check):
    """a Psi script from the full run of every step-halving problem: after each Newton step halvings[k] values that keep
    falling, then one that rises (the step is accepted) -- after the last step one that repeats the previous iterate's
    (converged).  The loop must halve as often per step as the mirror did and report its iters and converged."""
    lines, want = [], []
    for kind in H.KINDS:
        ref = H.reference(kind, "full")
        assert ref["converged"] and len(ref["halvings"]) == ref["iters"] and sum(ref["halvings"]) >= 2
        psis, prev = [0.0], 0.0
        for k, nh in enumerate(ref["halvings"]):
            psis += [prev - 8.0 - i for i in range(nh)]
            prev = prev if k + 1 == len(ref["halvings"]) else prev + 8.0
            psis.append(prev)
        lines.append(run_line(TOL, H.max_iter_of(kind, "full"), psis))
        want.append((list(ref["halvings"]), ref["iters"], int(ref["converged"]), 0))
    got = []
    for line in state_check("iterate", lines):
        trace, iters, converged, status = parse_run(line)
        runs = " ".join(trace).split("forward")[1:]                 # one piece per forward product
        assert all(r.split()[0] == "eval0" and r.split().count("eval0") == 1 for r in runs), trace
        assert [r.split()[-1] for r in runs] == ["step"] * (len(runs) - 1) + ["factor1"], trace
        got.append(([r.split().count("eval1") for r in runs[1:]], iters, converged, status))
    assert got == want
