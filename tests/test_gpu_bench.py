"""bench.py's command line: a plain run's result line and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(tmp_path):
    """One small plain run (256 envs x 32 steps, 3 timed iterations): the line carries the
    headline fields, ms_per_step is the time of one of the --steps timed iterations (value is
    the env-steps of one iteration over it), nothing that --full adds was measured, and
    --dump-outputs wrote the last iteration's arrays as float32 / float64 .npy files."""
    E, Tn, K = 256, 32, 3
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1",
                        "--envs", str(E), "--horizon", str(Tn), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == K and d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    # value and ms_per_step are two roundings (0.1 env-steps/s, 1 us) of one elapsed time
    assert d["value"] == pytest.approx(E * Tn * 1e3 / d["ms_per_step"], rel=2e-3 / d["ms_per_step"] + 1e-6)
    assert "cpu_baseline" not in d and d["roofline_gae"] is None

    arrs = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out)) if f.endswith(".npy")}
    assert {"policy_theta", "vf_theta", "stats", "batch_rows", "batch_obs", "batch_act", "batch_prob", "batch_rew",
            "batch_flags", "batch_vpred", "batch_adv", "batch_ret"} <= set(arrs)
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert all(np.isfinite(a).all() for a in arrs.values())
    rows = arrs["batch_rows"]
    assert len(rows) == E * Tn and (np.diff(rows) > 0).all()  # small batch: every row, in order
    assert arrs["batch_obs"].shape == (E * Tn, 11) and arrs["batch_act"].shape == (E * Tn, 3)
    # the advantages are the standardised ones the update consumed (numpy std, ddof = 0)
    adv = arrs["batch_adv"].astype(np.float64)
    assert abs(adv.mean()) < 1e-4 and abs(adv.std() - 1.0) < 1e-4
    with open(out / "stats_names.json") as f:
        assert len(json.load(f)) == len(arrs["stats"]) > 0
