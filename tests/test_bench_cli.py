"""bench.py command line: the result line, --dump-outputs and --full (CPU
plumbing configuration — tiny models, 2000 docs)."""

import json
import os
import subprocess
import sys

import numpy as np


def test_bench_dump_outputs_and_full_cpu(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = tmp_path / "dump"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    proc = subprocess.run(
        [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "0", "--full",
         "--dump-outputs", str(out_dir)],
        capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["metric"] == "chat_qps" and res["value"] > 0
    assert res["unit"] == "requests/s" and res["higher_is_better"] is True
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    batch = res["config"]["global_batch"]
    # value and ms_per_step describe the same timed steps
    assert abs(res["value"] - batch / (res["ms_per_step"] / 1e3)) \
        <= 0.02 * res["value"]

    names = {p.name for p in out_dir.iterdir()}
    assert names == {"query_embeddings.npy", "dense_scores.npy",
                     "sparse_scores.npy", "fused_scores.npy"}
    total = 0
    for p in out_dir.iterdir():
        a = np.load(p)
        assert a.dtype == np.float32, (p.name, a.dtype)
        assert a.size > 0 and np.isfinite(a).all(), p.name
        total += a.nbytes
    assert total <= 64 << 20
    # shapes follow from the arguments (top-k 10), never from the data
    assert np.load(out_dir / "query_embeddings.npy").shape[0] == batch
    for name in ("dense_scores", "sparse_scores", "fused_scores"):
        a = np.load(out_dir / (name + ".npy"))
        assert a.shape == (batch, 10), name
        assert (np.diff(a, axis=1) <= 0).all(), name     # descending
    assert (np.load(out_dir / "dense_scores.npy") != 0).any()
