"""bench.py launches its own ranks when --gpus N > 1 and WORLD_SIZE is unset
(the driver's `python3 bench.py --gpus 8` shape).  --dry rehearses that
launcher and the int16-as-bytes gather on CPU with gloo (trivial host compute,
no GPU): the gathered global batch must hold every rank's frames in order."""
import json
import os

import pytest
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=240)


@pytest.mark.parametrize("n", [2, 4, 8])  # the driver's scaling sweep shapes (N = 1 is the GPU bench)
def test_bench_spawns_ranks_and_gathers(n):
    r = _run(["--dry", "--gpus", str(n), "--width", "96", "--height", "48", "--frames", "2",
              "--steps", "1", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == n and res["global_batch"] == 2 * n and res["gather"] == "gloo"
    assert res["gathered_frames_ok"] == f"{2 * n}/{2 * n}"


def test_dump_outputs_float32_and_size_limit(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy files, whole while they fit the limit, else
    the same sample of the flattened elements in every run."""
    import numpy as np
    import bench
    a = (np.arange(7 * 33 * 65) % 2048 - 16).astype(np.int16).reshape(7, 33, 65)
    bench.dump_outputs(str(tmp_path / "whole"), {"disparity": a})
    got = np.load(tmp_path / "whole" / "disparity.npy")
    assert got.dtype == np.float32 and got.shape == a.shape and np.array_equal(got, a)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 16 * 1024)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"disparity": a})
    s1, s2 = (np.load(tmp_path / d / "disparity.npy") for d in ("s1", "s2"))
    assert s1.dtype == np.float32 and s1.ndim == 1 and 0 < s1.size < a.size
    assert os.path.getsize(tmp_path / "s1" / "disparity.npy") <= 16 * 1024
    assert np.array_equal(s1, s2) and np.isin(s1, a).all()


def test_bench_rejects_world_size_mismatch():
    r = _run(["--dry", "--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE" in r.stderr
