"""bench.py's command line on the host engine at a tiny scale factor: a plain run reports the
headline only and honours ``--steps``; ``--dump-outputs`` writes the last timed step's results."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_reports_headline_only_and_dumps_last_step(tmp_path):
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--device", "cpu",
           "--sf", "0.02", "--steps", "3", "--warmup", "1", "--buckets", "4",
           "--data-dir", str(tmp_path / "data"), "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "queries/s" and out["higher_is_better"] is True and out["dtype"] == "fp64"
    assert out["ms_per_step"] > 0
    # value = 2 queries per step / seconds per step (both rounded to 3 places in the record)
    assert abs(out["value"] - 2000.0 / out["ms_per_step"]) <= 1e-3 * out["value"] + 1e-3
    # the side measurements and checks belong to --full
    for key in ("latency", "crosscheck", "q3_full", "q3_3way", "hybrid", "join_index", "replicated"):
        assert key not in out, key
    assert "cold first queries" not in r.stderr
    names = sorted(os.listdir(dump))
    assert names == ["q3_lines.npy", "q3_o_shippriority.npy", "q3_revenue.npy", "q6_revenue.npy"]
    arrs = {n[:-4]: np.load(dump / n) for n in names}
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in arrs.values())
    assert arrs["q6_revenue"].shape == (1,) and np.isfinite(arrs["q6_revenue"][0])
    n = len(arrs["q3_revenue"])
    assert n >= 1 and len(arrs["q3_lines"]) == n and len(arrs["q3_o_shippriority"]) == n
    assert (arrs["q3_lines"] >= 1).all() and (arrs["q3_revenue"] > 0).all()
