"""The route table of the kernel-matrix build's GPU tests (kbuild_route_table.py) against the one function that decides
which kernel a launch reaches (gaussian_process_amd/csrc/gpmi_kroute.h: rbf_route), under g++ AddressSanitizer + UBSan.
No GPU.

tests/sanitize/kbuild_route_check.cpp answers (kind, d, shape, bounding box, rbf_blocks) queries with the kernel's name,
the launch geometry and the tile forms, holds every grid against a direct count of the tiles the launch owes, and
checks the triangular tile enumeration by brute force."""
import os
import shutil
import subprocess

import pytest

import kbuild_route_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def route_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("kroute") / "kbuild_route_check")
    subprocess.check_call([shutil.which("g++"), "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gaussian_process_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "kbuild_route_check.cpp")])

    def ask(queries):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe], input="".join(q + "\n" for q in queries), env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        return lines
    return ask


def query(case, **more):
    """the launch as the entry point of the case turns it into an RbfArgs (gpmi_api.hip: cov_impl, dev_api.hip)"""
    c = case._replace(**more)
    words = [c.kind, c.d, c.nA + int(c.far), c.nB, c.nrows, c.ncols, int(c.api == "rows"), c.row0, float(T.coef(c)).hex(),
             float(T.max_sq(c)).hex(), T.RBF_BLOCKS if c.blocks is None else c.blocks]
    return " ".join(str(w) for w in words)


def parse(line):
    name, rest = line.split("|")
    tri, strip, nitems, grid, lds, nocheck, interior, edge, diag, skipped = (int(w) for w in rest.split())
    forms = {f for f, n in (("interior", interior), ("edge", edge), ("diag", diag), ("skipped", skipped)) if n}
    return dict(kernel=name, tri=tri, strip=strip, nitems=nitems, grid=grid, lds=lds, nocheck=nocheck, forms=frozenset(forms))


@pytest.fixture(scope="module")
def answers(route_check):
    claims = T.all_claims()
    return claims, [parse(a) for a in route_check([query(c.case) for c in claims])]


def test_every_case_reaches_what_the_table_claims(answers):
    claims, got = answers
    wrong = []
    for c, g in zip(claims, got):
        want = dict(kernel=c.kernel, tri=c.tri, strip=c.strip, nocheck=c.nocheck, forms=c.forms)
        have = {k: g[k] for k in want}
        if have != want:
            wrong.append("%s:\n  table       %s\n  rbf_route   %s" % (c.case, want, have))
    assert not wrong, "\n".join(wrong)
    for c, g in zip(claims, got):
        if c.case.blocks is not None:           # the persistent loop runs: more work items than blocks
            assert g["grid"] == c.case.blocks < g["nitems"], (c.case, g)


def test_every_instantiation_and_form_is_claimed():
    claims = T.all_claims()
    claimed = {c.kernel for c in claims}
    assert claimed == set(T.INSTANTIATIONS)
    for F in range(4):
        for D in T.REG_D:
            forms = set().union(*(c.forms for c in claims if c.kernel == T.regs_name(D, F)))
            assert {"interior", "edge", "diag"} <= forms, (F, D, forms)
        # each specialisation of the interior loop, in every family
        inner = {T.interior_form(c) for c in claims if c.kernel.startswith("rbf_regs_kernel") and c.kernel.endswith(", %d>" % F)
                 and "interior" in c.forms}
        assert inner == {"check_unit", "check_sigma", "nocheck_unit", "nocheck_sigma"}, (F, inner)
    # the three launch shapes, the persistent loop with skipped items, the 4-tile strip
    regs = [c for c in claims if c.kernel.startswith("rbf_regs_kernel")]
    assert any(c.tri for c in regs) and any(c.case.api == "rows" and c.case.row0 > 0 for c in regs)
    assert any(c.case.api != "rows" for c in regs)
    assert {c.case.blocks for c in regs if "skipped" in c.forms} >= {1, 3, 7, 64}
    assert any(c.strip == 4 and c.tri for c in regs) and any(c.strip == 4 and not c.tri for c in regs)


def test_nocheck_threshold_from_both_sides():
    """the bounding box's worst argument is about -689.9 (nocheck) or -690.1 (check), and an element takes it"""
    import numpy as np
    import matern_ref as M
    for c in T.THRESHOLD:
        A, B = T.inputs(c.case)
        sq = M.sq_cross(A, B)
        arg = T.coef(c.case) * (sq if c.case.kind == 0 else np.sqrt(sq))
        box = T.coef(c.case) * (T.max_sq(c.case) if c.case.kind == 0 else np.sqrt(T.max_sq(c.case)))
        assert arg.min() == box and arg.min() >= -700.0
        assert abs(box - (-689.9 if c.nocheck else -690.1)) < 1e-9, box


def test_triangular_enumeration_by_brute_force(route_check):
    assert route_check(["tri"]) == ["tri ok %d" % (1024 * 1025 // 2)]


def test_refusals_and_the_largest_launch(route_check):
    C = T.Case
    big = C("rows", 0, 8, 131072, 131072, 0, 131072, 131072)            # 1024 x 1024 tiles: the triangle is 524800 tiles
    got = [parse(a) for a in route_check([query(big), query(big, blocks=3),
                                          query(C("cov", 0, 3, 300, 512), nrows=0), query(C("cov", 0, 3, 300, 512), nrows=130),
                                          query(C("rows", 0, 3, 450, 450, 64, 256, 512)), query(C("cov", 2, 1, 300, 512), d=2),
                                          query(C("cov", 0, 3, 300, 512), kind=7)])]
    assert got[0]["kernel"] == T.regs_name(8, 0) and got[0]["tri"] == 1 and got[0]["strip"] == 4
    assert got[0]["nitems"] == 256 * 1024 and got[0]["grid"] == T.RBF_BLOCKS and got[1]["grid"] == 3
    assert [g["kernel"] for g in got[2:]] == ["nothing", "invalid", "invalid", "invalid", "invalid"]
