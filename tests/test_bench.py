"""bench.py's command line: --steps, --dump-outputs (what the last timed step handed its caller, as .npy files), and --full
(everything the benchmark measures beyond its headline figure)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench(args, timeout):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=timeout)


# keys of the single-GPU line that only --full adds
FULL_ONLY = ("other_call_form", "roofline", "stages_ms", "kbuild_hbm", "alpha_hbm", "peaks_probe", "peaks_box", "targets",
             "seconds_incl_transfers")


def test_bench_rejects_no_timed_steps_cpu():
    p = _bench(["--steps", "0"], timeout=60)
    assert p.returncode != 0 and "--steps" in p.stderr


def test_bench_knows_full_cpu():
    """--full is an option of its own (the command line is parsed before anything needs a GPU)"""
    p = _bench(["--full", "--steps", "0"], timeout=60)
    assert p.returncode != 0 and "--steps must be at least 1" in p.stderr and "unrecognized" not in p.stderr


def test_dump_outputs_bound_and_sample_cpu(tmp_path, monkeypatch):
    """under the bound every array is written whole in float64; past it each keeps a seeded sample of its elements
    in index order, the same from run to run, and the files stay within the bound"""
    import bench
    rng = np.random.default_rng(3)
    arrays = {"lml": 12.5, "mu": rng.standard_normal(300), "var": rng.random(300), "alpha": rng.standard_normal(5000)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "whole" / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, np.asarray(v, dtype=np.float64))
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 8000)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    assert sum(np.load(tmp_path / "a" / (k + ".npy")).nbytes for k in arrays) <= 8000
    for k, v in arrays.items():
        a, b = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert np.array_equal(a, b)
        full = np.asarray(v, dtype=np.float64).reshape(-1)
        pos = [int(np.flatnonzero(full == x)[0]) for x in a.reshape(-1)]
        assert pos == sorted(pos)                       # elements of the output, in index order


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_timed_step_results(tmp_path, oracle):
    """--dump-outputs at a small size: lml, mu, var and alpha of the last timed step as float64 .npy files, equal to the
    result line's lml and to the oracle on the bench's seeded inputs; --steps sets the number of timed steps"""
    N, d, n = 2048, 8, 128
    out = tmp_path / "dump"
    p = _bench(["--gpus", "1", "--size", str(N), "--dim", str(d), "--ntest", str(n), "--steps", "2", "--warmup", "1",
                "--no-cpu-baseline", "--no-other-form", "--dump-outputs", str(out)], timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    got = {k: np.load(out / (k + ".npy")) for k in ("lml", "mu", "var", "alpha")}
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["mu"].shape == (n,) and got["var"].shape == (n,) and got["alpha"].shape == (N,)
    assert float(got["lml"]) == line["lml"]
    X, y, Xs = oracle.synthetic_problem(N, d, n)
    ref = oracle.fit_predict_feasible(X, Xs, y, 1.0, 2.0, 5e-4, use_c=False)
    assert np.max(np.abs(got["mu"] - ref["mu"])) < 1e-9
    assert np.max(np.abs(got["var"] - ref["var"])) < 1e-10
    assert abs(float(got["lml"]) - ref["lml"]) < 1e-10 * abs(ref["lml"])
    assert np.max(np.abs(got["alpha"] - ref["alpha"])) < 1e-8 * np.max(np.abs(ref["alpha"]))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_full_adds_the_rest(tmp_path):
    """a plain run prints the headline line alone; --full prints the same headline with what the benchmark measures
    beyond it, and the timed steps hand back the same bits either way"""
    args = ["--gpus", "1", "--size", "2048", "--dim", "8", "--ntest", "128", "--steps", "2", "--warmup", "1"]
    lines = {}
    for form, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        p = _bench(args + extra + ["--dump-outputs", str(tmp_path / form)], timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        out = [l for l in p.stdout.splitlines() if l.strip()]
        assert len(out) == 1, p.stdout[-2000:]
        lines[form] = json.loads(out[0])
    plain, full = lines["plain"], lines["full"]
    for line in (plain, full):
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "seconds", "steps", "warmup",
                    "config", "lml"):
            assert key in line, key
        assert line["unit"] == "TFLOP/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert plain["metric"] == full["metric"] and plain["config"]["call_form"] == full["config"]["call_form"]
    assert not set(plain) & set(FULL_ONLY + ("cpu_baseline", "extra_configs")), sorted(plain)
    assert set(FULL_ONLY) <= set(full), sorted(full)
    assert full["other_call_form"]["lml_equal"] and full["other_call_form"]["alpha_equal"]
    assert plain["lml"] == full["lml"]
    for k in ("lml", "mu", "var", "alpha"):
        assert np.array_equal(np.load(tmp_path / "plain" / (k + ".npy")), np.load(tmp_path / "full" / (k + ".npy"))), k
