"""-m gpu: the plain bench line and --dump-outputs (small configuration, one GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("xyz", "opacity", "scaling", "rotation", "shs")


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--config", "small", "--prime-seconds", "0", "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_times_its_steps_and_dumps_the_last_step(dev, tmp_path):
    j = _bench(tmp_path / "a")
    assert j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "img/s" and j["higher_is_better"] is True
    assert j["dtype"] == "f32" and j["value"] > 0
    assert abs(j["ms_per_step"] - 1e3 * j["config"]["bsz_per_gpu"] / j["value"]) < 0.01 * j["ms_per_step"]
    # a plain run measures the headline only: the extra passes and legs need --full
    assert j["value_gt_streamed"] is None and j["value_instrumented"] is None and not j["kernels"]
    assert "cpu_baseline" not in j and "host_resident" not in j and "trainer" not in j and "heavy" not in j
    a = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(a) == {"losses", "sparsity", *FIELDS}, sorted(a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in a.values())
    assert a["losses"].shape == (j["config"]["bsz_per_gpu"],)
    n = a["xyz"].shape[0]
    assert n == min(j["config"]["n_gaussians"], 1 << 17)
    assert [a[k].shape for k in FIELDS] == [(n, 3), (n, 1), (n, 3), (n, 4), (n, 48)]
    # the same arguments give the same inputs: a second run trains to the same state (float atomics reorder sums)
    _bench(tmp_path / "b")
    for k in a:
        np.testing.assert_allclose(np.load(tmp_path / "b" / f"{k}.npy"), a[k], rtol=1e-3, atol=1e-3, err_msg=k)
