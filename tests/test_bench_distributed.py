"""Distributed bench path on CPU: 2 ranks over gloo, exactly the code the
driver runs with torch.distributed.run on GPU nodes (RCCL there)."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_bench_two_rank_gloo(tmp_path):
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    # force the CPU/gloo path even on a GPU box: two ranks sharing one GPU
    # is not a supported RCCL topology (the driver gives each rank its own)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29571", str(REPO / "bench.py"),
         "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "16",
         "--no-verify"],
        capture_output=True, text=True, timeout=600, env=env, cwd=str(REPO))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    result = json.loads(lines[0])
    assert result["metric"] == "pods_scheduled_per_sec"
    assert result["n_gpus"] == 2
    assert result["value"] > 0
    assert result["scaling"] == "weak"
    assert result["config"]["global_batch"] == 32


def test_bench_single_rank_json_contract():
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--steps", "2",
         "--warmup", "1", "--batch", "16", "--no-verify"],
        capture_output=True, text=True, timeout=600, cwd=str(REPO))
    assert out.returncode == 0, out.stderr[-3000:]
    result = json.loads([l for l in out.stdout.splitlines()
                         if l.startswith("{")][0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in result, key
    assert result["n_gpus"] == 1
    assert result["data"] == "synthetic"


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's results as .npy, and the
    same arguments give the same inputs, hence identical outputs, in two
    separate processes (--full on one of them must not change them)."""
    import numpy as np

    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out_dir = tmp_path / name
        out = subprocess.run(
            [sys.executable, str(REPO / "bench.py"), "--steps", "3",
             "--warmup", "1", "--batch", "16", "--no-verify",
             "--dump-outputs", str(out_dir)] + extra,
            capture_output=True, text=True, timeout=600, cwd=str(REPO))
        assert out.returncode == 0, out.stderr[-3000:]
        result = json.loads([l for l in out.stdout.splitlines()
                             if l.startswith("{")][0])
        assert result["steps"] == 3
        assert result["ms_per_step"] > 0
        dumps.append({p.stem: np.load(p) for p in out_dir.glob("*.npy")})
    a, b = dumps
    assert set(a) == {"feasible", "scores", "bound_node", "cards"}
    assert set(b) == set(a)
    for name, arr in a.items():
        assert arr.dtype in (np.float32, np.float64), name
        assert arr.shape[0] == 16, name
        assert np.array_equal(arr, b[name]), name
    # every pod was bound to a feasible node and holds at least one card
    rows = np.arange(16)
    nodes = a["bound_node"].astype(int)
    assert (nodes >= 0).all()
    assert (a["feasible"][rows, nodes] == 1).all()
    assert (a["scores"][rows, nodes] >= 0).all()
    assert (a["cards"].sum(axis=1) >= 1).all()
