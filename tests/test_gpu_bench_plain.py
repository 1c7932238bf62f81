"""bench.py's plain line on one GPU (fresh child processes): exactly --steps timed steps, the headline keys and nothing that --full
adds, and --dump-outputs writing the same arrays in two runs with the same arguments (seeded inputs, bit-reproducible plan)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-settle",
           "--img", "64", "--z", "32", "--batch-per-gpu", "8", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(tmp_path):
    d = _run(tmp_path / "a")
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"} <= set(d)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["settle_steps"] == 0 and d["dtype"] == "bf16x3"
    assert d["unit"] == "images/sec" and d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) <= 0.02 * d["value"]
    assert not {"roofline", "variants", "exact_f32", "cpu_baseline"} & set(d)          # --full only
    a = {p[:-4]: np.load(tmp_path / "a" / p) for p in os.listdir(tmp_path / "a")}
    assert {"loss", "recon", "kl", "x_tilde", "mu", "logvar", "param.decoder.conv.0.conv.weight"} <= set(a)
    assert a["x_tilde"].shape == (8, 3, 64, 64) and a["mu"].shape == (8, 32)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert abs(float(a["loss"]) - d["loss"]) <= 1e-3 * abs(d["loss"])
    _run(tmp_path / "b")
    b = {p[:-4]: np.load(tmp_path / "b" / p) for p in os.listdir(tmp_path / "b")}
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
