"""bench.py's command line: a plain run prints the headline line without the
--full measurements, --steps sets the number of timed updates, and
--dump-outputs writes the last timed update's outputs as float32 .npy files
within its size limit."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "kernels", "separate_sim_ms_per_update", "cpu_baseline")
DUMPED = ("params", "values", "rewards", "dones", "advantages", "bootstrap", "actions",
          "log_probs", "metrics")


@pytest.mark.gpu
def test_plain_run_line_and_dump(gpu, tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "2", "--warmup", "2", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["ms_per_step"] > 0
    # value = env-steps of one update / seconds of one update
    assert d["value"] == pytest.approx(65536 * 32 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert not any(k in d for k in FULL_ONLY)

    files = sorted(os.listdir(out))
    assert files == sorted(n + ".npy" for n in DUMPED)
    total = 0
    for n in DUMPED:
        a = np.load(out / (n + ".npy"))
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), n
        total += os.path.getsize(out / (n + ".npy"))
    assert total <= 64 * 1000 * 1000
    # the update ran: a rollout was stored and the parameters are not all zero
    assert np.load(out / "bootstrap.npy").shape == (65536,)
    assert np.abs(np.load(out / "params.npy")).max() > 0
    assert np.abs(np.load(out / "values.npy")).max() > 0
