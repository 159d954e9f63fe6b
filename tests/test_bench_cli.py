"""bench.py's command line on the reduced-dims model, each run a fresh process: a plain run prints the headline line and nothing else,
``--steps`` sets the timed steps, and ``--dump-outputs`` writes what the last timed step returned - the same arrays run after run, and
the same whether or not ``--full`` calibrated thresholds and ran the on-policy leg before the timed region."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("on_policy", "latency_ms_by_exit", "scripted", "surface", "roofline", "batched", "batched_groups", "window",
             "batched_max_envs", "cpu_baseline")


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--workload", "tiny",
           "--dump-outputs", str(out_dir), *extra]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def _dumped(d):
    return {n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_same_outputs_as_a_full_run(tmp_path):
    lines = [_bench(tmp_path / "a"), _bench(tmp_path / "b"),
             _bench(tmp_path / "full", "--full", "--calib-steps", "24", "--burn-in", "0", "--on-policy-steps", "6", "--no-cpu-baseline",
                    "--batched-envs", "0", "--surface-steps", "0", "--no-roofline", "--latency-reps", "0", "--scripted-steps", "0")]
    for out in lines:
        assert out["steps"] == 7 and out["warmup"] == 2 and sum(out["config"]["exit_hist"]) == 7
        assert out["unit"] == "action-steps/s" and out["higher_is_better"] is True and out["value"] > 0 and out["ms_per_step"] > 0
        assert abs(out["ms_per_step"] * out["value"] - 1e3) < 10.0                 # ms_per_step: one timed step
    assert not [k for k in FULL_ONLY if k in lines[0] or k in lines[1]]
    assert "on_policy" in lines[2] and lines[2]["config"]["thresholds"] is not None
    a, b, full = _dumped(tmp_path / "a"), _dumped(tmp_path / "b"), _dumped(tmp_path / "full")
    assert {"pose.npy", "gripper.npy", "exit_layer.npy", "deltas.npy"} <= set(a) and set(a) == set(b) == set(full)
    for n, x in a.items():
        assert x.dtype in (np.float32, np.float64) and x.shape[0] == 1, (n, x.dtype, x.shape)
        assert np.array_equal(x, b[n]) and np.array_equal(x, full[n]), n
