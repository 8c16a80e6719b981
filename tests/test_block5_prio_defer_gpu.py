"""mlp_block5's default step schedule against the previous schedule's own instantiation (DCT_B5_SCHED=0,
csrc/knobs.h) at the launch boundaries.  Round 10's schedule items were per-phase wave priorities (no value
changes; kept, in the default) and the W2 / b1 / b2 owners' Adam of step s deferred into step s + 1, in front
of barrier A: it carried that step's gradient sums and Adam scalars, was skipped in a launch's first step and
flushed after its last one.  The deferred update measured slower and was removed; the
cases are the ones set for it, since what a schedule item that carries state across steps gets wrong is
launch boundaries and the carried scalars: launches of one step (every step first and last), 2 + 1, 63 + 3
(the second launch straddles the 64-step block of the Adam-scalar table) and 40 + 30 with a short last batch.
Every value keeps its instruction sequence: parameters, moments and per-step losses must be equal bit for
bit.  The generic LDS trainer is the independent reference that keeps the knob from selecting nothing."""
import functools
import math

import pytest
import torch

import dct_amd  # noqa: F401
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import FusedMLPKernel

pytestmark = pytest.mark.gpu

# (dims, batch)
SHAPES = {"5in-b4": ([5, 128, 128, 2], 4),
          "8in-b3": ([8, 128, 128, 2], 3),
          "1in-b1": ([1, 128, 128, 2], 1)}
# steps of each launch, rows missing in the last batch (batch 1 has none to miss)
SPLITS = {"7x1": ([1] * 7, 0),
          "2+1": ([2, 1], 0),
          "63+3": ([63, 3], 0),
          "40+30-short": ([40, 30], 1)}
MAX_STEPS = 70
# (dropout, loss, weight decay): the whole cross on the headline shape, two opposite corners on the others
OPTIONS = [(d, l, w) for d in (0.0, 0.2) for l in ("ce", "mse") for w in (0.0, 0.01)]
CORNERS = [(0.2, "ce", 0.01), (0.0, "mse", 0.0)]
CASES = [(shape, split) + opt for shape in SHAPES for split in SPLITS
         for opt in (OPTIONS if shape == "5in-b4" else CORNERS)]


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
    dims, B = SHAPES[shape]
    g = torch.Generator().manual_seed(29)
    N = 2 * MAX_STEPS * B + 7
    X = torch.randn(N, dims[0], generator=g).cuda()
    Y = torch.randint(0, dims[-1], (N,), generator=g).to("cuda", torch.int32)
    idx = torch.randperm(N, generator=g)[:MAX_STEPS * B].to("cuda", torch.int32)
    return X, Y, idx, _flat_params(dims, 13).cuda()


def _train(monkeypatch, env, shape, split, dropout, loss, wd):
    """The split's launches under env (a value of None: unset); returns (p, m, v, losses) on the CPU."""
    for k_, v_ in env.items():
        if v_ is None:
            monkeypatch.delenv(k_, raising=False)
        else:
            monkeypatch.setenv(k_, v_)
    dims, B = SHAPES[shape]
    launches, short = SPLITS[split]
    steps = sum(launches)
    n_items = steps * B - min(short, B - 1)
    assert math.ceil(n_items / B) == steps <= MAX_STEPS
    X, Y, idx, p0 = _data(shape)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    losses = torch.zeros(steps, device=p0.device)
    k = FusedMLPKernel(dims, bmax=4)  # (re-reads the knobs)
    assert k.plan.trainer(B) == ("lds" if env.get("DCT_MLP_BLOCK") == "0" else "block5")  # the kernel under test
    first = 0
    for n in launches:
        k.train(p, m, v, X, Y, idx[first * B:n_items], n_items=n_items - first * B, batch=B, steps=n, t0=first, lr=0.01,
                weight_decay=wd, dropout=dropout, seed=3, step_base=first, loss=loss, loss_out=losses[first:])
        first += n
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu(), losses.cpu()


DEFAULT = {"DCT_B5_SCHED": None, "DCT_MLP_KERNEL": None, "DCT_MLP_BLOCK": None}


@pytest.mark.parametrize("shape,split,dropout,loss,wd", CASES,
                         ids=["-".join(str(x) for x in c) for c in CASES])
def test_block5_default_schedule_equals_sched0_at_launch_boundaries(shape, split, dropout, loss, wd, cuda, monkeypatch):
    new = _train(monkeypatch, DEFAULT, shape, split, dropout, loss, wd)
    old = _train(monkeypatch, dict(DEFAULT, DCT_B5_SCHED="0"), shape, split, dropout, loss, wd)
    for name, a_, b_ in zip("pmvl", new, old):
        assert torch.isfinite(a_).all(), name
        assert torch.equal(a_, b_), (name, float((a_ - b_).abs().max()))
    assert bool((new[3] != 0).all())  # every step of every launch wrote its loss


def test_block5_default_schedule_matches_lds_trainer_across_launches(cuda, monkeypatch):
    """Default schedule against the generic LDS trainer (same dropout hash, loss and Adam, another summation
    order) over the 63 + 3 launches, at the tolerance of tests/test_block5_sched_gpu.py."""
    case = ("5in-b4", "63+3", 0.2, "ce", 0.01)
    new = _train(monkeypatch, DEFAULT, *case)
    ref = _train(monkeypatch, dict(DEFAULT, DCT_MLP_KERNEL="lds", DCT_MLP_BLOCK="0"), *case)
    for a_, b_ in zip(new, ref):
        assert torch.isfinite(a_).all()
        err = float((a_ - b_).abs().max())
        print(f"max|new - lds| = {err:.3e} (bound {1e-4 * (1 + float(b_.abs().max())):.3e})")
        assert err <= 1e-4 * (1 + b_.abs().max())
