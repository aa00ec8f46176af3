"""bench.py --dump-outputs: after the timed steps the line's run writes what its last timed step produced (the step's losses, a
fixed sample of the updated parameters) as float32 .npy files, 64 MB at most; the same arguments give the same inputs from run
to run, and --steps is the number of steps the dump reflects."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--model", "tiny", "--input-size", "64", "--num-encoded-tokens", "24", "--batch", "8", "--warmup", "1", "--no-cpu-baseline",
        "--legs", "none", "--tunable", "0", "--block-timer", "0"]


def _bench(steps, out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--dump-outputs", str(out_dir)] + ARGS,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(out_dir):
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_bench_dump_outputs(tmp_path):
    a = _bench(3, tmp_path / "a")
    b = _bench(3, tmp_path / "b")
    c = _bench(4, tmp_path / "c")
    assert (a["steps"], b["steps"], c["steps"]) == (3, 3, 4)
    da, db, dc = _load(tmp_path / "a"), _load(tmp_path / "b"), _load(tmp_path / "c")
    assert sorted(k + ".npy" for k in da) == a["dump_outputs"]["files"]
    assert {"loss", "loss_contra", "s1_loss", "s2_loss", "dem_loss", "params"} <= set(da)
    assert all(v.dtype in (np.float32, np.float64) for v in da.values())
    assert sum(v.nbytes for v in da.values()) <= 64 << 20
    assert np.isfinite(da["params"]).all() and da["params"].size == a["dump_outputs"]["params_dumped"]
    assert abs(float(da["loss"]) - a["config"]["loss"]) <= 1e-4
    # same arguments: same weights, inputs and mask draws -> the same step, up to the order of floating-point reductions
    for k in da:
        assert da[k].shape == db[k].shape, k
    assert abs(float(da["loss"]) - float(db["loss"])) <= 1e-3 * abs(float(da["loss"]))
    # one more timed step moves the parameters by far more than the run-to-run spread
    run_to_run = np.abs(da["params"] - db["params"]).mean()
    one_step = np.abs(da["params"] - dc["params"]).mean()
    assert one_step > 0 and run_to_run < 0.1 * one_step, (run_to_run, one_step)
