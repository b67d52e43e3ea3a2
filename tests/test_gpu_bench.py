"""bench.py as a command: a plain run (no --full) prints one JSON line with the headline alone, and
--dump-outputs writes the results of the last timed step, which agree with the line's own summary of them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

E = 8192


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--edges", str(E), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "interpolants/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # value = rake_early_exit interpolants of one step / the step's time
    assert line["value"] == pytest.approx(line["config"]["interpolants_per_gpu"] / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("cpu_baseline", "parity", "full_mask", "roofline_hbm_fk"):  # the legs behind --full
        assert line[k] is None, k
    assert sorted(os.listdir(out)) == ["n_e.npy", "ok.npy"]
    ok, n_e = np.load(out / "ok.npy"), np.load(out / "n_e.npy")
    assert ok.dtype == np.float32 and n_e.dtype == np.float32 and ok.shape == (E,) and n_e.shape == (E,)
    assert set(np.unique(ok)) <= {0.0, 1.0} and n_e.min() >= 0 and np.all(n_e == np.round(n_e))
    assert ok.mean(dtype=np.float64) == pytest.approx(line["config"]["edge_valid_fraction"], abs=1e-6)
    assert n_e.mean(dtype=np.float64) == pytest.approx(line["config"]["mean_n_e"], abs=1e-6)
