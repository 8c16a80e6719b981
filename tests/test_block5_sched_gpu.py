"""mlp_block5's step schedule (DCT_B5_SCHED, csrc/knobs.h): the default schedule moves gradient-free
work of the step (next step's dropout factors, Adam's per-step scalars as a 64-step lane table, one
block of dZ1's W1 transposes, the next input tile's read) out of the contended backward.  Every value
keeps its instruction sequence, so parameters, moments and losses must equal the previous schedule's
(DCT_B5_SCHED=0) bit for bit; the generic LDS trainer is the independent reference."""
import math

import pytest
import torch

import dct_amd  # noqa: F401
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import FusedMLPKernel

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_knobs():
    native().reload_knobs()


def _flat_params(dims, seed):
    g = torch.Generator().manual_seed(seed)
    parts = []
    for i in range(len(dims) - 1):
        bound = 1.0 / math.sqrt(dims[i])
        parts.append((torch.rand(dims[i + 1], dims[i], generator=g) * 2 - 1) * bound)
        parts.append((torch.rand(dims[i + 1], generator=g) * 2 - 1) * bound)
    return torch.cat([t.reshape(-1) for t in parts])


def _data(dims, n_items, cuda):
    g = torch.Generator().manual_seed(17)
    N = 2 * n_items + 7
    X = torch.randn(N, dims[0], generator=g).to(cuda)
    Y = torch.randint(0, dims[-1], (N,), generator=g).to(cuda, torch.int32)
    idx = torch.randperm(N, generator=g)[:n_items].to(cuda, torch.int32)
    return X, Y, idx, _flat_params(dims, 5).to(cuda)


def _train(monkeypatch, env, data, dims, B, n_items, launches, dropout, loss, wd):
    """launches: [(first step, steps, t0, step_base)], consecutive; returns (p, m, v, losses) on the CPU."""
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    X, Y, idx, p0 = data
    steps = math.ceil(n_items / B)
    assert sum(n for _, n, _, _ in launches) == steps
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    losses = torch.zeros(steps, device=p0.device)
    k = FusedMLPKernel(dims, bmax=4)  # (re-reads the knobs)
    assert k.plan.trainer(B) == ("lds" if env.get("DCT_MLP_BLOCK") == "0" else "block5")  # the kernel under test
    for first, n, t0, sbase in launches:
        k.train(p, m, v, X, Y, idx[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=t0, lr=0.01,
                weight_decay=wd, dropout=dropout, seed=3, step_base=sbase, loss=loss, loss_out=losses[first:])
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu(), losses.cpu()


def _assert_same(new, old):
    for a_, b_ in zip(new, old):
        assert torch.isfinite(a_).all()
        assert torch.equal(a_, b_), float((a_ - b_).abs().max())


# 131 steps of batch 4 (the last one has 3 rows): the 64-step table of Adam scalars refreshes twice.
# Two launches of 70 + 61 steps: the second starts at a step count that is no multiple of 64.
TWO = [(0, 70, 0, 0), (70, 61, 70, 70)]
ONE = [(0, 131, 3, 5)]


@pytest.mark.parametrize("launches", [TWO, ONE], ids=["two-launches", "t0-3-base-5"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dropout", [0.0, 0.2])
def test_block5_schedule_equals_previous_bitwise(dropout, loss, wd, launches, cuda, monkeypatch):
    dims, B, n_items = [5, 128, 128, 2], 4, 523
    data = _data(dims, n_items, cuda)
    new = _train(monkeypatch, {"DCT_B5_SCHED": "1"}, data, dims, B, n_items, launches, dropout, loss, wd)
    old = _train(monkeypatch, {"DCT_B5_SCHED": "0"}, data, dims, B, n_items, launches, dropout, loss, wd)
    _assert_same(new, old)


@pytest.mark.parametrize("dims,B,n_items", [([8, 128, 128, 2], 3, 200), ([1, 128, 128, 2], 1, 70)])
@pytest.mark.parametrize("split", [True, False], ids=["two-launches", "t0-3-base-5"])
def test_block5_schedule_equals_previous_other_shapes(dims, B, n_items, split, cuda, monkeypatch):
    """Eight inputs at batch 3 (67 steps, the last with 2 rows) and one input at batch 1 (70 steps)."""
    steps = math.ceil(n_items / B)
    launches = [(0, 40, 0, 0), (40, steps - 40, 40, 40)] if split else [(0, steps, 3, 5)]
    data = _data(dims, n_items, cuda)
    new = _train(monkeypatch, {"DCT_B5_SCHED": "1"}, data, dims, B, n_items, launches, 0.2, "ce", 0.01)
    old = _train(monkeypatch, {"DCT_B5_SCHED": "0"}, data, dims, B, n_items, launches, 0.2, "ce", 0.01)
    _assert_same(new, old)


def test_block5_schedule_matches_lds_trainer(cuda, monkeypatch):
    """The default schedule against the generic LDS trainer (an independent kernel: same dropout hash,
    loss and Adam, another summation order) over the 131 steps - the knob must not select nothing."""
    dims, B, n_items = [5, 128, 128, 2], 4, 523
    data = _data(dims, n_items, cuda)
    new = _train(monkeypatch, {"DCT_B5_SCHED": "1"}, data, dims, B, n_items, ONE, 0.2, "ce", 0.0)
    ref = _train(monkeypatch, {"DCT_MLP_KERNEL": "lds", "DCT_MLP_BLOCK": "0"}, data, dims, B, n_items, ONE, 0.2,
                 "ce", 0.0)
    for a_, b_ in zip(new, ref):
        assert torch.isfinite(a_).all()
        err = float((a_ - b_).abs().max())
        print(f"max|new - lds| = {err:.3e} (bound {1e-4 * (1 + float(b_.abs().max())):.3e})")
        assert err <= 1e-4 * (1 + b_.abs().max())
