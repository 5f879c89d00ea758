"""GPU: the one JSON line `python bench.py` prints (the driver's contract) -- a short run of the default
configuration, checked for every field the contract names and their relations: value = rollouts per second of the
timed steps (N / ms_per_step), the workload BASELINE's metric is quoted on, and with --full the roofline of the step's
launch (achieved = the algorithmic bytes of one launch over its event-timed duration, frac = achieved / peak) and the
CPU baseline's fields.  A plain run carries the headline fields only and, with --dump-outputs, writes the last timed
step's outputs, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("device_chain", "armed_step", "python_step", "kernels_us", "roofline", "cpu_baseline", "north_star_65536",
             "c3", "c5_1gpu", "interface_step", "tamols_c4", "c4")


def run_bench(*extra):
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "50", "--warmup", "5", *extra]
    p = subprocess.run(args, cwd=ROOT, capture_output=True, text=True, timeout=200)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]  # one line on stdout (native banners go to stderr)
    return json.loads(lines[0])


def check_headline(d):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "p50_step_ms", "p99_step_ms",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["metric"] == "SRBD rollouts/sec + p50 MPC-step ms at N=10k H=12; 1/2/4/8 GPU"
    assert d["unit"] == "rollouts/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert (d["n_gpus"], d["steps"], d["warmup"]) == (1, 50, 5)
    assert d["scaling"] == "weak" and d["dtype"] == "f32" and "synthetic" in d["data"]
    c = d["config"]
    assert c["workload"] == "go2_trot_flat_mppi_n10000_h12_zo" and c["num_samples"] == 10000 and c["horizon"] == 12
    assert (c["method"], c["parametrization"]) == ("mppi", "zero_order")
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - c["num_samples"] / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """Without --full: the headline fields only, p50 / p99 over the metric's 1 000-step sample; --dump-outputs writes
    the last timed step's outputs (float32 / float64 .npy), bit-identical between two runs with the same arguments,
    and the second pass that collects them reproduces the timed step's parameters."""
    runs = []
    for name in ("a", "b"):
        d = run_bench("--dump-outputs", str(tmp_path / name))
        check_headline(d)
        assert d["full"] is False and d["latency_steps"] == 1000 and len(d["timed_step_us"]) == 50
        assert not [k for k in FULL_ONLY if k in d]
        assert 0 < d["p50_step_ms"] <= d["p99_step_ms"]
        info = d["dump_outputs"]
        assert info["replay_bitwise"] is True
        assert info["arrays"] == {"best": [144], "best_cost": [1], "best_index": [1], "costs": [10000], "grf": [12],
                                  "predicted_state": [24]}
        arrs = {n: np.load(tmp_path / name / (n + ".npy")) for n in info["arrays"]}
        assert sorted(os.listdir(tmp_path / name)) == sorted(n + ".npy" for n in arrs)
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert all(np.isfinite(a).all() for n, a in arrs.items() if n != "costs")  # a diverged rollout costs NaN
        assert sum(a.nbytes for a in arrs.values()) == info["bytes"] <= 64 << 20
        # the step's own relations: the best rollout's cost is the smallest of the step's costs, at its index
        i = int(arrs["best_index"][0])
        assert arrs["costs"][i] == np.nanmin(arrs["costs"]) == arrs["best_cost"][0]
        assert np.abs(arrs["grf"]).max() > 0
        runs.append(arrs)
    for n, a in runs[0].items():
        np.testing.assert_array_equal(a, runs[1][n], err_msg=n)


def test_bench_default_line_contract():
    d = run_bench("--full", "--latency-steps", "50", "--device-steps", "50", "--other-steps", "0", "--targets", "0",
                  "--extras", "0", "--cpu-seconds", "0.5")
    assert d["full"] is True
    check_headline(d)
    assert "roofline" in d and "cpu_baseline" in d
    c = d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["algorithmic_bytes_per_launch"] == c["num_samples"] * r["bytes_per_rollout"] == 5_800_000
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["kernel_us"] * 1e3)) <= 0.01 * r["achieved"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) <= 1e-4
    assert r["traffic"] is None or r["traffic"] > 0
    assert 0 < r["kernel_us"] * 1e-3 < d["ms_per_step"]  # the launch fits inside the host step it is part of
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["unit"] == "rollouts/s" and cb["value"] > 0 and cb["cores"] >= 1
