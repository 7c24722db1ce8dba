"""A plain `bench.py` run (no --full) does only what its result line needs: set up, warm up, time the steps, write --dump-outputs,
print.  No CPU leg, no streaming copy / fill, no secondary list: those belong to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_alone(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["metric"] == "Msamples/s (whole node) for 65536-voice SVF+FM graph"
    assert res["unit"] == "Msamples/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["value"] > 0 and res["ms_per_step"] > 0 and res["roofline"]["kernel_ms_avg"] > 0
    assert res["cpu_baseline"] is None and res["roofline"]["measured_streaming"] is None and res["config"]["scaling_alt"] is None
    assert '"secondary"' not in r.stderr
    out = np.load(tmp_path / "out.npy")
    assert out.shape[:2] == (1, 48000) and np.isfinite(out).all()
