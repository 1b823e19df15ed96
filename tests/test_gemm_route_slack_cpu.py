"""Sharing::panel_slack, the state of a Cholesky whose lookahead panel chain has slack (49152 columns and more), in the one
route function (gaussian_process_amd/csrc/gpmi_route.h: gemm_route), under g++ AddressSanitizer + UBSan.  No GPU.

In the state the bar of the 256 x 128 form is tall_min_tiles_slack instead of tall_min_tiles; out of it gemm_route answers
for every (route, case) of gemm_route_table.py what the table says -- whatever tall_min_tiles_slack is."""
import os
import shutil
import subprocess

import pytest

import gemm_route_table as T
import test_gemm_route_cpu as R

ROOT = R.ROOT
G = R.MI355X_GROUPS


@pytest.fixture(scope="module")
def slack_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("route_slack") / "gemm_route_slack_check")
    subprocess.check_call([shutil.which("g++"), "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gaussian_process_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "gemm_route_slack_check.cpp")])

    def ask(queries):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe], input="".join(q + "\n" for q in queries), env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        names = p.stdout.splitlines()
        assert len(names) == len(queries)
        return names
    return ask


def query(slack, groups, name, case, role=0, **kw):
    words = R.query(groups, name, case, **kw).split()
    words[3] = str(role)
    return " ".join([str(int(slack))] + words)


def test_state_off_every_case_reaches_the_kernel_the_table_names(slack_check):
    """out of the state: the table's answer with and without a counter pool, at the default tall_min_tiles_slack, at 0
    (which in the state would send every per-tile launch to the 256 x 128 form) and at a bar nothing reaches"""
    for more in ({}, {"tall_min_tiles_slack": 0}, {"tall_min_tiles_slack": 1 << 30}):
        for groups, want in ((G, lambda n, c: T.kernel(n, c)), (0, lambda n, c: T.NO_POOL.get(n, T.kernel(n, c)))):
            got = slack_check([query(0, groups, n, c, **more) for n, c in R.LAUNCHED])
            wrong = ["%s-%s %s: want %s, gemm_route %s" % (n, c, more, want(n, c), g)
                     for (n, c), g in zip(R.LAUNCHED, got) if g != want(n, c)]
            assert not wrong, "\n".join(wrong)


def test_state_on_touches_nothing_but_the_bar(slack_check):
    """in the state with tall_min_tiles_slack = the route's tall_min_tiles: the table's answer for every (route, case)"""
    qs = [query(1, G, n, c, tall_min_tiles_slack=dict(T.DEFAULTS, **T.ROUTES[n][0])["tall_min_tiles"]) for n, c in R.LAUNCHED]
    got = slack_check(qs)
    wrong = ["%s-%s: want %s, gemm_route %s" % (n, c, T.kernel(n, c), g) for (n, c), g in zip(R.LAUNCHED, got) if g != T.kernel(n, c)]
    assert not wrong, "\n".join(wrong)


def test_the_slack_bar_from_both_sides(slack_check):
    C = T.Case
    dma8, tall = T.ROUTES["dma8"][2], T.ROUTES["tall"][2]
    dma8_trail, tall_trail = "chol_trailing_update_dma_kernel", "chol_trailing_update_dma256_kernel"
    beside = dict(sharing=(1, 1))                   # cholesky_inplace under lookahead: Sharing::beside_update
    own = dict(beside, tall_min_tiles=12288)        # route "tall" with the default bar outside the state
    rows = 65536 + 128 + 4096                       # the headline's matrix: N, the y rows, the test set's rows
    want = [
        # the option, in the state: the lower triangle of 16 x 16 tiles holds 136 live tiles
        (query(1, G, "tall", C(2048, 2048, 48, lower=1), tall_min_tiles_slack=136, **own), tall),
        (query(1, G, "tall", C(2048, 2048, 48, lower=1), tall_min_tiles_slack=137, **own), dma8),
        # ... and out of it, where tall_min_tiles alone decides
        (query(0, G, "tall", C(2048, 2048, 48, lower=1), tall_min_tiles_slack=136, **own), dma8),
        (query(0, G, "tall", C(2048, 2048, 48, lower=1), tall_min_tiles_slack=137, tall_min_tiles=136, **beside), tall),
        (query(1, G, "tall", C(2048, 2048, 48, lower=1), tall_min_tiles_slack=137, tall_min_tiles=0, **beside), dma8),
        # the default, 1024: 32 x 32 tiles reach it, 32 x 31 do not; out of the state 12288 = 96 x 128 tiles do, 95 x 128 do not
        (query(1, G, "small_dma3", C(4096, 4096, 256)), tall), (query(1, G, "small_dma3", C(4096, 3968, 256)), dma8),
        (query(0, G, "small_dma3", C(4096, 4096, 256)), dma8),
        (query(0, G, "small_dma3", C(12288, 16384, 256)), tall), (query(0, G, "small_dma3", C(12160, 16384, 256)), dma8),
        (query(1, G, "small_dma3", C(12160, 16384, 256)), tall),
        # gemm_tall 0 and the 4-wave kernel keep the 128 x 128 form in the state as well
        (query(1, G, "small_dma3", C(4096, 4096, 256), gemm_tall=0), dma8),
        (query(1, G, "small_dma3", C(4096, 4096, 256), gemm_dma_waves=4), "gemm_nt_dma_kernel<4, false>"),
        # the launches of the headline factorisation (block 2048): the next-block-column launches ...
        (query(1, G, "small_dma3", C(rows - 2048, 2048, 2048, lower=1)), tall), (query(0, G, "small_dma3", C(rows - 2048, 2048, 2048, lower=1)), dma8),
        # (136 + 16 live tiles per tile row below the square: the bar is 72 tile rows, which the last two launches miss)
        (query(1, G, "small_dma3", C(rows - 59392, 2048, 2048, lower=1)), tall), (query(1, G, "small_dma3", C(rows - 61440, 2048, 2048, lower=1)), dma8),
        (query(1, G, "small_dma3", C(rows - 63488, 2048, 2048, lower=1)), dma8),
        (query(1, G, "small_dma3", C(rows - 2048, 2048, 2048, lower=1), role=1), tall_trail),
        (query(0, G, "small_dma3", C(rows - 2048, 2048, 2048, lower=1), role=1), dma8_trail),
        # ... a late rest-of-the-update launch (8192 columns left: 2080 + 40 x 64 live tiles) ...
        (query(1, G, "small_dma3", C(rows - 57344, 8192, 2048, lower=1), role=1), tall_trail),
        (query(0, G, "small_dma3", C(rows - 57344, 8192, 2048, lower=1), role=1), dma8_trail),
        # ... and the updates inside the first panel: K = 1024 and 512 are above the bar, K = 256 (2 x 542 tiles) is on
        # it only for the first panels, K = 128 never; few tiles stay on the 64 x 64 kernel
        (query(1, G, "small_dma3", C(rows - 1024, 1024, 1024, lower=1)), tall), (query(0, G, "small_dma3", C(rows - 1024, 1024, 1024, lower=1)), dma8),
        (query(1, G, "small_dma3", C(rows - 512, 512, 512, lower=1)), tall),
        (query(1, G, "small_dma3", C(rows - 256, 256, 256, lower=1)), tall), (query(1, G, "small_dma3", C(128 * 512, 256, 256, lower=1)), dma8),
        (query(1, G, "small_dma3", C(rows - 128, 128, 128, lower=1)), dma8),
        (query(1, G, "small_dma3", C(1024, 1024, 48)), "gemm_nt_small_kernel<3>"),
    ]
    got = slack_check([q for q, _ in want])
    wrong = ["%s: want %s, gemm_route %s" % (q, w, g) for (q, w), g in zip(want, got) if g != w]
    assert not wrong, "\n".join(wrong)
