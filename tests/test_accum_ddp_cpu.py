"""accumulate_grad_batches under DDP on the CPU (two gloo processes, autograd engine, torch bucket reducer): one
gradient all-reduce per optimizer step, of the accumulated gradient (Lightning's no_sync on the other micro-batches),
replicas identical, and the trajectory of a single-process emulation."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import dct_amd  # noqa: F401
from dct_amd.data.sampler import distributed_indices
from dct_amd.data.synthetic import weather_tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "accum_ddp_worker.py")
B, K = 4, 7


def _emulate(rows, epochs, world, lr=0.01):
    """Per rank and window: sum of (1 / K) * grad of each micro-batch's own mean CE; the ranks' sums averaged; one Adam
    step per window (the worker's split and sampler seeds)."""
    from dct_amd.models.mlp import MLPClassifier

    torch.manual_seed(42)
    x, y = weather_tensors(rows, seed=0)
    n_tr = int(0.8 * rows)
    tr_idx = torch.randperm(rows)[:n_tr]
    model = MLPClassifier(5, hidden=(64,), dropout=0.0)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    params = list(model.parameters())
    steps = 0
    for ep in range(epochs):
        shards = [tr_idx[distributed_indices(n_tr, world, r, shuffle=True, seed=42, epoch=ep)] for r in range(world)]
        nb = math.ceil(len(shards[0]) / B)
        for w0 in range(0, nb, K):
            gs = [torch.zeros_like(p) for p in params]
            for sh in shards:
                for b in range(w0, min(w0 + K, nb)):
                    rows_b = sh[b * B:(b + 1) * B]
                    loss = F.cross_entropy(model(x[rows_b]), y[rows_b]) / K  # always 1 / K, also in the short window
                    for a, g in zip(gs, torch.autograd.grad(loss, params)):
                        a += g
            for p, g in zip(params, gs):
                p.grad = g / world
            opt.step()
            steps += 1
    return torch.cat([p.detach().reshape(-1) for p in params]), steps


@pytest.mark.slow
def test_two_rank_gloo_ddp_accumulates_and_reduces_once_per_step(tmp_path):
    rows, epochs = 600, 2
    e = dict(os.environ)
    e.pop("CUDA_VISIBLE_DEVICES", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", "--master-port=29671", "--max-restarts=0", WORKER, str(tmp_path), str(epochs),
           str(rows), str(K)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = [json.loads((tmp_path / f"params_rank{k}.json").read_text()) for k in (0, 1)]
    p0, p1 = (torch.tensor(o["params"]) for o in out)
    assert torch.equal(p0, p1), (p0 - p1).abs().max()
    want, steps = _emulate(rows, epochs, 2)
    nb = math.ceil(240 / B)
    assert nb % K != 0 and steps == epochs * math.ceil(nb / K) == 18
    err = float((p0 - want).abs().max())
    print("2-rank accumulating fit vs the emulation: max |dp| = %.3e" % err)
    assert err < 1e-4  # tests/test_ddp_cpu.py's tolerance for the same comparison at K = 1
    for o in out:
        assert o["engine"] == "autograd" and o["reducer"] == "TorchBucketReducer" and o["global_step"] == steps
        # the reducer ran once per optimizer step, and only that micro-batch's hooks handed it gradients
        assert o["finalize"] == steps and o["mark_ready"] == steps * o["n_params"]
    assert out[0]["train_loss"] == pytest.approx(out[1]["train_loss"])  # the cross-rank mean
