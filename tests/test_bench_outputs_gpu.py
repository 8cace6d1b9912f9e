"""A plain `bench.py --gpus 1 --steps K --warmup W` run: the headline line and nothing the --full run adds, K timed steps, and
--dump-outputs giving the same files in two runs with the same arguments (the clip is seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"roofline", "path_roofline", "kernel_roofline", "kernel_ms_per_step", "kernel_traffic", "power", "cpu_baseline",
             "jod_delta_vs_reference", "jod_delta_vs_oracle_sample"}


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "fhd64",
           "--frames", "24", "--gen", "gpu", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, env=dict(os.environ, CVVDP_BENCH_SPINUP_S="0.3"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_dumps_the_same_outputs_every_time(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    lines = [_plain_run(a), _plain_run(b)]
    for d in lines:
        assert d["metric"] == "Mpixels/s" and d["unit"] == "Mpixel/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and 0 < d["jod"] <= 10
        assert abs(d["value"] - 1920 * 1080 * 24 / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"]
        assert not FULL_ONLY & set(d), FULL_ONLY & set(d)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and {"jod.npy", "Q_per_ch.npy", "rho_band.npy"} <= set(names)
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(x, y, err_msg=n)
    assert np.load(a / "Q_per_ch.npy").shape[2] == 24                       # every frame of the clip
    assert abs(float(np.load(a / "jod.npy")) - lines[0]["jod"]) <= 1e-5
