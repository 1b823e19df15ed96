"""The pair plans of the 256 x 128 GEMM form (gaussian_process_amd/csrc/gpmi_plan.h) under g++ AddressSanitizer + UBSan,
held against brute force by tests/sanitize/pair_plan_check.cpp. No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pair_planner_under_asan_ubsan(tmp_path):
    """Every live 128-tile covered by exactly one live half of one block, no dead tile written, no doubly dead block in a
    diagonal supertile, the 128-tile plan's supertiles kept, blocks priced at two tiles."""
    exe = str(tmp_path / "pair_plan_check")
    subprocess.check_call([shutil.which("g++"), "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "gaussian_process_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "pair_plan_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert "pair_plan_check: ok" in p.stdout
