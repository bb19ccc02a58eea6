"""bench.py's plain run as every change measures it: one JSON line with the headline fields and
nothing behind --full, and --dump-outputs writing the last timed step's targets within budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_dumps_outputs(gpu, tmp_path):
    dump = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out, key
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["config"]["render_errors"] == 0
    # the --full measurements stay out of a plain run
    assert out["roofline"] is None
    for key in ("rooflines", "one_frame_per_step", "single_stream", "concurrent_streams_one_gpu",
                "cpu_baseline"):
        assert key not in out, key

    pool = out["config"]["pool"]
    names = sorted(os.listdir(dump))
    assert names == sorted(f"target_{i}.npy" for i in range(pool)), names
    assert sum(os.path.getsize(dump / n) for n in names) <= 64 << 20
    first = None
    for n in names:
        a = np.load(dump / n)
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 4, (n, a.shape, a.dtype)
        assert np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0
        assert np.unique(a[:, 3]).size == 1     # one alpha: the frame is opaque
        first = a.shape if first is None else first
        assert a.shape == first
