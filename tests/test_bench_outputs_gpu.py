"""The plain benchmark line and `--dump-outputs`: a run without `--full` carries the headline contract and none of the extra
measurements, and two runs with the same arguments write the same outputs of the last timed step (seeded inputs, deterministic kernels)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

B, P, T = 3, 24, 12


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--tiny",
           "--prompt-tokens", str(P), "--new-tokens", str(T), "--batch-per-gpu", str(B), "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _load(d):
    got = {}
    for name in ("actions", "token_ids", "lens"):
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        got[name] = a
    return got


def test_plain_line_and_dumped_outputs_are_reproducible(device, tmp_path):
    d = _run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in d, k
    assert d["metric"] == "actions/sec" and d["unit"] == "actions/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - B * 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    for k in ("roofline", "cpu_baseline", "stage_us", "rccl_ranks", "single_gpu_same_workload"):
        assert k not in d, k                      # behind --full
    a = _load(tmp_path / "a")
    assert a["actions"].shape == (B, 7) and np.isfinite(a["actions"]).all()
    assert a["token_ids"].shape == (B, T) and (a["token_ids"] >= 0).all() and (a["token_ids"] == np.round(a["token_ids"])).all()
    assert (a["lens"] == T).all()
    _run(tmp_path / "b")
    b = _load(tmp_path / "b")
    for name in a:
        assert np.array_equal(a[name], b[name]), name
