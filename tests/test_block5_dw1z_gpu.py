"""mlp_block5's default step schedule against the previous schedule's own instantiation (DCT_B5_SCHED=0,
csrc/knobs.h) on the shapes, step splits and options below.  The schedule items only move work inside the
step - the default issues one W1 k-block's quad transposes for dZ1 right behind barrier B, under the loss,
and W1 is rewritten by Adam only at the end of the step - so every value keeps its instruction sequence and
parameters, moments and per-step losses must be equal bit for bit.  The interleaved dZ1 / dW1 / Adam
backward this file was first written for measured slower and was removed; the
cases are the ones set for it.  The generic LDS trainer is the independent reference that keeps the knob
from selecting nothing."""
import functools
import math

import pytest
import torch

import dct_amd  # noqa: F401
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import FusedMLPKernel

pytestmark = pytest.mark.gpu

STEPS, FIRST = 70, 40  # two launches, 40 + 30 steps: the second starts at a step count that is no multiple of 64
# (dims, batch, items): 70 steps each; the last step of the first two is one row short
SHAPES = {"5in-b4": ([5, 128, 128, 2], 4, 69 * 4 + 3),
          "8in-b3": ([8, 128, 128, 2], 3, 69 * 3 + 2),
          "1in-b1": ([1, 128, 128, 2], 1, 70)}


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


@functools.lru_cache(maxsize=None)
def _data(shape):
    """Inputs, labels, batch order and start parameters of one shape (shared by its cases, never written)."""
    dims, _, n_items = SHAPES[shape]
    g = torch.Generator().manual_seed(23)
    N = 2 * n_items + 7
    X = torch.randn(N, dims[0], generator=g).cuda()
    Y = torch.randint(0, dims[-1], (N,), generator=g).to("cuda", torch.int32)
    idx = torch.randperm(N, generator=g)[:n_items].to("cuda", torch.int32)
    return X, Y, idx, _flat_params(dims, 11).cuda()


def _train(monkeypatch, env, shape, dropout, loss, wd):
    """Both launches under env (a value of None: unset); returns (p, m, v, losses) on the CPU."""
    for k_, v_ in env.items():
        if v_ is None:
            monkeypatch.delenv(k_, raising=False)
        else:
            monkeypatch.setenv(k_, v_)
    dims, B, n_items = SHAPES[shape]
    assert math.ceil(n_items / B) == STEPS
    X, Y, idx, p0 = _data(shape)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    losses = torch.zeros(STEPS, device=p0.device)
    k = FusedMLPKernel(dims, bmax=4)  # (re-reads the knobs)
    assert k.plan.trainer(B) == ("lds" if env.get("DCT_MLP_BLOCK") == "0" else "block5")  # the kernel under test
    for first, n in ((0, FIRST), (FIRST, STEPS - FIRST)):
        k.train(p, m, v, X, Y, idx[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=first, lr=0.01,
                weight_decay=wd, dropout=dropout, seed=3, step_base=first, loss=loss, loss_out=losses[first:])
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu(), losses.cpu()


DEFAULT = {"DCT_B5_SCHED": None, "DCT_MLP_KERNEL": None, "DCT_MLP_BLOCK": None}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dropout", [0.0, 0.2])
def test_block5_default_schedule_equals_sched0_bitwise(dropout, loss, wd, shape, cuda, monkeypatch):
    new = _train(monkeypatch, DEFAULT, shape, dropout, loss, wd)
    old = _train(monkeypatch, dict(DEFAULT, DCT_B5_SCHED="0"), shape, dropout, loss, wd)
    for name, a_, b_ in zip("pmvl", new, old):
        assert torch.isfinite(a_).all(), name
        assert torch.equal(a_, b_), (name, float((a_ - b_).abs().max()))
    assert float(new[3].abs().max()) > 0.0  # the launches wrote their losses


def test_block5_default_schedule_matches_lds_trainer(cuda, monkeypatch):
    """Default schedule against the generic LDS trainer (same dropout hash, loss and Adam, another summation
    order), at the tolerance of tests/test_block5_sched_gpu.py."""
    new = _train(monkeypatch, DEFAULT, "5in-b4", 0.2, "ce", 0.01)
    ref = _train(monkeypatch, dict(DEFAULT, DCT_MLP_KERNEL="lds", DCT_MLP_BLOCK="0"), "5in-b4", 0.2, "ce", 0.01)
    for a_, b_ in zip(new, ref):
        assert torch.isfinite(a_).all()
        err = float((a_ - b_).abs().max())
        print(f"max|new - lds| = {err:.3e} (bound {1e-4 * (1 + float(b_.abs().max())):.3e})")
        assert err <= 1e-4 * (1 + b_.abs().max())
