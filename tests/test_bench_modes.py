"""`bench.py` reports the timed steps alone; `bench.py --full` adds the oracle check of the timed buffers and every further
measurement (CPU baselines, per-kernel roofline, per-step spread, device copy, extras) to the same line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "roofline_hbm_bound", "kernels", "cpu_baseline", "cpu_baseline_multicore", "verified", "verification",
             "sampling_chain", "device_copy_GBps", "stack_frac_of_device_copy", "ms_per_step_min", "ms_per_step_median",
             "ms_per_step_max")


def _bench(extra, timeout):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "EPNET_BENCH_BATCH")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


def _line(extra):
    r = _bench(extra, 280)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.timeout(120)
def test_sweep_belongs_to_full():
    """--sweep times further runs: without --full it is refused rather than dropped"""
    r = _bench(["--sweep", "16"], 100)
    assert r.returncode != 0 and "--full" in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_line_is_the_headline_and_full_adds_the_rest(tmp_path):
    small = ["--batch", "8", "--steps", "3", "--warmup", "2"]
    plain = _line(small + ["--dump-outputs", str(tmp_path / "plain")])
    full = _line(small + ["--full", "--extras", "", "--cpu-scenes", "1", "--dump-outputs", str(tmp_path / "full")])
    assert plain["full"] is False and full["full"] is True
    assert all(key in plain for key in HEADLINE) and plain["value"] > 0 and plain["ms_per_step"] > 0
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[key] == full[key], key
    assert not set(FULL_ONLY) & set(plain), sorted(set(FULL_ONLY) & set(plain))
    assert set(FULL_ONLY) <= set(full), sorted(set(FULL_ONLY) - set(full))
    assert full["verified"] is True and full["kernels"] and full["cpu_baseline"]["value"] > 0
    # the same timed steps on the same inputs: both runs leave the same outputs behind
    names = sorted(plain["dumped_outputs"]["arrays"])
    assert names and names == sorted(full["dumped_outputs"]["arrays"])
    for name in names:
        a, b = (np.load(str(tmp_path / d / (name + ".npy"))) for d in ("plain", "full"))
        assert np.array_equal(a, b), name
