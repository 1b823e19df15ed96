"""The route table of the GPU tests (gemm_route_table.py) against the one function that decides which kernel a launch of the
update GEMM reaches (gaussian_process_amd/csrc/gpmi_route.h: gemm_route), under g++ AddressSanitizer + UBSan.  No GPU.

tests/sanitize/gemm_route_check.cpp answers (options, sharing state, shape) queries with the kernel's name, and holds every
plan, grid and LDS size of the LDS-DMA family against plan_tiles on the way."""
import os
import shutil
import subprocess

import pytest

import gemm_route_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI355X_GROUPS = 256         # resident workgroups of the counter pool: one per CU


@pytest.fixture(scope="module")
def route_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("route") / "gemm_route_check")
    subprocess.check_call([shutil.which("g++"), "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gaussian_process_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "gemm_route_check.cpp")])

    def ask(queries):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe], input="".join(q + "\n" for q in queries), env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        names = p.stdout.splitlines()
        assert len(names) == len(queries)
        return names
    return ask


def query(groups, name, case, sharing=None, **more):
    """a launch of gemm_contract.Buffers.launch as the C-ABI turns it into a GemmArgs (dev_api.hip), under the options and
    the sharing state of tests/test_gemm_routes_gpu.py: route (sharing: (small-LDS forms, chip shared) instead; more:
    options on top of the route's)"""
    opts, concurrent = T.ROUTES[name][:2]
    assert set(opts) <= set(T.DEFAULTS)
    opts = dict(opts, **more)
    small_lds, chip_shared = sharing if sharing is not None else (concurrent, concurrent)
    reach = case.reach or ()
    host = case.reach is not None and (case.host_map or case.brows > 0)      # a block table takes the map with its host copy
    words = [groups, int(small_lds), int(chip_shared), 0, len(opts)]
    for k, v in opts.items():
        words += [k, v]
    words += [case.M, case.N, case.K, case.lower, case.diag_off, case.rbr // 128, int(host), case.brows, len(reach), *reach]
    return " ".join(str(w) for w in words)


def pairs(table):
    return [(n, c) for n in table for c in (table[n][3] if table is T.ROUTES else table[n])]


# every (route, case) the GPU tests launch: the exact cases, the bound cases, and the forms compared bit for bit
LAUNCHED = pairs(T.ROUTES) + pairs(T.BOUND) + [(n, c) for n in ("dma8", "tall", "persist", "ticket")
                                               for c in (T.PERSIST[1], T.PERSIST[2], T.PERSIST[4])]


def test_every_case_reaches_the_kernel_the_table_names(route_check):
    got = route_check([query(MI355X_GROUPS, n, c) for n, c in LAUNCHED])
    wrong = ["%s-%s: table %s, gemm_route %s" % (n, c, T.kernel(n, c), g) for (n, c), g in zip(LAUNCHED, got) if g != T.kernel(n, c)]
    assert not wrong, "\n".join(wrong)
    # every kernel a route names is reached by at least one of its cases
    for name in T.ROUTES:
        assert any(g == T.ROUTES[name][2] for (n, _), g in zip(LAUNCHED, got) if n == name), name


def test_without_a_counter_pool(route_check):
    """no pool: the per-tile routes are untouched, the resident ones fall to one workgroup per tile"""
    got = route_check([query(0, n, c) for n, c in LAUNCHED])
    wrong = ["%s-%s: want %s, gemm_route %s" % (n, c, T.NO_POOL.get(n, T.kernel(n, c)), g)
             for (n, c), g in zip(LAUNCHED, got) if g != T.NO_POOL.get(n, T.kernel(n, c))]
    assert not wrong, "\n".join(wrong)


def test_thresholds_and_sharing_states(route_check):
    """each threshold of the decision from both sides, the ablation bits, and what the two sharing flags switch"""
    C = T.Case
    small8, small3 = "gemm_nt_small_kernel<8>", "gemm_nt_small_kernel<3>"
    dma8, tall, persist, ticket = (T.ROUTES[n][2] for n in ("dma8", "tall", "persist", "ticket"))
    G = MI355X_GROUPS
    want = [
        # half a round of 128 x 128 tiles: 127 tiles small, 128 on the LDS-DMA family
        (query(G, "small_dma8", C(16256, 128, 48)), small8), (query(G, "small_dma8", C(2048, 1024, 48)), dma8),
        # the persistent form: K >= 256 and two rounds of blocks (512: 24 x 24 tiles are 3 x 3 supertiles = 576 blocks,
        # 2560 x 2560 are 400 tiles in 9 supertiles of 64 too; 16 x 16 tiles are 256 blocks)
        (query(G, "persist", C(3072, 3072, 240)), dma8), (query(G, "persist", C(3072, 3072, 256)), persist),
        (query(G, "persist", C(2048, 2048, 256)), dma8), (query(G, "persist", C(4096, 2048, 256)), persist),
        # the ticket form: one round of blocks (15 x 16 tiles are 4 supertiles of 64: 256 blocks; 1664 x 1664: 4 supertiles)
        (query(G, "ticket", C(1920, 2048, 48)), ticket), (query(G, "ticket", C(1024, 2048, 48)), dma8),
        # the 256 x 128 form: at least tall_min_tiles live tiles (the lower triangle of 16 x 16 tiles holds 136)
        (query(G, "tall", C(2048, 2048, 48, lower=1), tall_min_tiles=136), tall),
        (query(G, "tall", C(2048, 2048, 48, lower=1), tall_min_tiles=137), dma8),
        (query(G, "tall", C(2048, 2048, 48), gemm_dma_waves=4), "gemm_nt_dma_kernel<4, false>"),
        # ablation bits: 1 .. 255 keep a launch off the LDS-DMA kernels and off the 64 x 64 ones, >= 256 only off the latter;
        # the low byte picks the probe instantiation and switches the resident forms off; the tall form stays chosen
        (query(G, "persist", C(2944, 2944, 256), gemm_dbg=1), "gemm_nt_kernel<4, 4, true>"),
        (query(G, "persist", C(2944, 2944, 256), gemm_dbg=256), persist),
        (query(G, "persist", C(2944, 2944, 256), gemm_dbg=272), "gemm_nt_dma_kernel<2, true>"),
        (query(G, "tall", C(2944, 2944, 256), gemm_dbg=272), "gemm_nt_dma_tall_kernel<true>"),
        (query(G, "dma4", C(2944, 2944, 256), gemm_dbg=272), "gemm_nt_dma_kernel<4, true>"),
        (query(G, "small_dma8", C(640, 640, 48), gemm_dbg=256), "gemm_nt_kernel<4, 4, true>"), (query(G, "small_dma8", C(640, 704, 48), gemm_dbg=1), "gemm_nt_kernel<4, 2, false>"),
        # sharing: the ring depth follows the small-LDS flag alone, the persistent form the chip-shared flag alone
        (query(G, "small_dma8", C(640, 640, 48), sharing=(0, 1)), small8), (query(G, "small_dma8", C(640, 640, 48), sharing=(1, 0)), small3),
        (query(G, "persist", C(2944, 2944, 256), sharing=(1, 0)), persist), (query(G, "persist", C(2944, 2944, 256), sharing=(0, 1)), dma8),
        # gemm_ticket 1 is for the Cholesky's own trailing updates (role 1, not reachable through the block primitives)
        (query(G, "ticket", C(2304, 2304, 48), sharing=(0, 1), gemm_ticket=1), dma8),
        # a block table goes to the LDS-DMA family whatever gemm_dma says and however few tiles; K = 16 cannot
        (query(G, "reg128", C(640, 640, 48, brows=128)), dma8), (query(G, "dma8", C(1536, 1920, 16, brows=256)), "invalid"),
        (query(G, "dma8", C(1536, 1920, 48, brows=192)), "invalid"),
        # nothing to launch: a staircase without a live supertile
        (query(G, "dma8", C(1920, 1920, 48, reach=(0,) * 15)), "nothing"), (query(G, "dma8", C(1920, 1920, 48, reach=(0,) * 15, host_map=False)), dma8),
    ]
    got = route_check([q for q, _ in want])
    wrong = ["%s: want %s, gemm_route %s" % (q, w, g) for (q, w), g in zip(want, got) if g != w]
    assert not wrong, "\n".join(wrong)
