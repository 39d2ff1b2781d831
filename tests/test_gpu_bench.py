"""``bench.py`` on one GPU: the plain run's result line, ``--steps`` as the number of timed rounds, and
``--dump-outputs`` (the last timed round's global model, metric and client losses as ``.npy`` files)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from attackfl_amd.models import ParamLayout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_result_line_and_dumped_outputs(gpu, tmp_path):
    dump = tmp_path / "dump"
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
           "--steps", "3", "--warmup", "1", "--full", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=150, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["rounds_ok"] == 3  # --steps rounds were timed
    assert out["unit"] == "rounds/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["value"] > 0 and out["ms_per_step"] == pytest.approx(1000.0 / out["value"], rel=1e-3)
    assert out["config"]["trainer"] == "fused"  # the native on-chip trainer, not an eager fallback
    got = {f: np.load(dump / f) for f in sorted(os.listdir(dump))}
    assert sorted(got) == ["client_loss.npy", "global_params.npy", "metric.npy"]
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    g, m, cl = got["global_params.npy"], got["metric.npy"], got["client_loss.npy"]
    assert g.dtype == np.float32 and g.shape == (ParamLayout.for_model("TransformerModel").P,)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    assert m.dtype == np.float64 and m.shape == (1,) and round(float(m[0]), 4) == out["test_roc_auc"]
    assert cl.dtype == np.float64 and cl.shape == (8, 5) and np.isfinite(cl).all() and (cl > 0).all()
