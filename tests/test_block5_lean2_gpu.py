"""mlp_block5's default step schedule against the previous schedule's own instantiation (DCT_B5_SCHED=0,
csrc/knobs.h), bit for bit: parameters, both Adam moments and every step's loss.  Round 12's items
(csrc/mlp_block5_impl.h, SCH_LOGIT_RS, SCH_INV_BS, SCH_ADAM_B02): the logit shares as a reduce-scatter, 1 / bs
once per launch with the per-step form behind a scalar branch for a short batch, b0 and b2 as one packed Adam
pair updated at the dW0 / db0 tail (b2 published there).  Every value keeps its operation sequence.  Cases: three shapes, the launch splits of tests/test_block5_lean_gpu.py, last batches of
1, 2 and 3 rows at batch 4 - inside a multi-step launch, as a dataset of that batch alone (one one-step
launch) and as the first step of a launch that follows a full one -, cross-entropy and MSE, weight decay 0
and 0.01, dropout 0, 0.2 and 0.5.  One case also checks that b0 and b2 moved from their start values, so the
comparison cannot pass on parameters nothing touched.  The generic LDS trainer is the independent reference
that keeps the knob from selecting nothing."""
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
# steps of each launch, rows missing in the last batch
SPLITS = {"7x1": ([1] * 7, 0),
          "2+1": ([2, 1], 0),
          "63+3": ([63, 3], 0),
          "40+30": ([40, 30], 0)}
MAX_STEPS = 70
# (dropout, loss, weight decay): the whole cross on the headline shape, two opposite corners on the others
OPTIONS = [(d, l, w) for d in (0.0, 0.2, 0.5) for l in ("ce", "mse") for w in (0.0, 0.01)]
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


def _bias_slices(dims):
    """Flat-parameter slices of b0 and b2 (torch order: W0, b0, W1, b1, W2, b2)."""
    b0 = dims[1] * dims[0]
    b2 = b0 + dims[1] + dims[2] * dims[1] + dims[2] + dims[3] * dims[2]
    return slice(b0, b0 + dims[1]), slice(b2, b2 + dims[3])


@functools.lru_cache(maxsize=None)
def _data(shape):
    """Inputs, labels, batch order and start parameters of one shape (shared by its cases, never written)."""
    dims, B = SHAPES[shape]
    g = torch.Generator().manual_seed(43)
    N = MAX_STEPS * B
    X = torch.randn(N, dims[0], generator=g).cuda()
    Y = torch.randint(0, dims[-1], (N,), generator=g).to("cuda", torch.int32)
    idx = torch.randperm(N, generator=g).to("cuda", torch.int32)
    return X, Y, idx, _flat_params(dims, 23).cuda()


def _run(monkeypatch, env, shape, n_items, launches, dropout, loss, wd):
    """The launches over the first n_items rows of the shape's batch order under env (a value of None: unset);
    returns (p, m, v, losses) on the CPU."""
    for k_, v_ in env.items():
        if v_ is None:
            monkeypatch.delenv(k_, raising=False)
        else:
            monkeypatch.setenv(k_, v_)
    dims, B = SHAPES[shape]
    steps = sum(launches)
    assert math.ceil(n_items / B) == steps <= MAX_STEPS
    X, Y, perm, p0 = _data(shape)
    idx = perm[:n_items]
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    losses = torch.zeros(steps, device=p0.device)
    k = FusedMLPKernel(dims, bmax=4)  # (re-reads the knobs)
    assert k.plan.trainer(B) == ("lds" if env.get("DCT_MLP_BLOCK") == "0" else "block5")  # the kernel under test
    first = 0
    for n in launches:
        k.train(p, m, v, X, Y, idx[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=first, lr=0.01,
                weight_decay=wd, dropout=dropout, seed=5, step_base=first, loss=loss, loss_out=losses[first:])
        first += n
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu(), losses.cpu()


DEFAULT = {"DCT_B5_SCHED": None, "DCT_MLP_KERNEL": None, "DCT_MLP_BLOCK": None}
SCHED0 = dict(DEFAULT, DCT_B5_SCHED="0")


def _assert_same(new, old):
    for name, a_, b_ in zip("pmvl", new, old):
        assert torch.isfinite(a_).all(), name
        assert torch.equal(a_, b_), (name, float((a_ - b_).abs().max()))
    assert bool((new[3] != 0).all())  # every step of every launch wrote its loss


@pytest.mark.parametrize("shape,split,dropout,loss,wd", CASES,
                         ids=["-".join(str(x) for x in c) for c in CASES])
def test_block5_lean2_schedule_equals_sched0(shape, split, dropout, loss, wd, cuda, monkeypatch):
    dims, B = SHAPES[shape]
    launches, _ = SPLITS[split]
    n_items = sum(launches) * B
    _assert_same(_run(monkeypatch, DEFAULT, shape, n_items, launches, dropout, loss, wd),
                 _run(monkeypatch, SCHED0, shape, n_items, launches, dropout, loss, wd))


# last batches of 1, 2 and 3 rows at batch 4: (launches, rows of the dataset)
def _short(kind, rows):
    if kind == "in-launch":        # the last step of a 30-step launch
        return [40, 30], 69 * 4 + rows
    if kind == "only-batch":       # the dataset is the short batch: one one-step launch
        return [1], rows
    assert kind == "first-step"    # a launch of full batches, then one that starts with the short batch
    return [6, 1], 6 * 4 + rows


SHORT_CASES = [(kind, rows) + opt for kind in ("in-launch", "only-batch", "first-step") for rows in (1, 2, 3)
               for opt in CORNERS + [(0.5, "ce", 0.0)]]


@pytest.mark.parametrize("kind,rows,dropout,loss,wd", SHORT_CASES,
                         ids=["-".join(str(x) for x in c) for c in SHORT_CASES])
def test_block5_lean2_short_last_batch_equals_sched0(kind, rows, dropout, loss, wd, cuda, monkeypatch):
    launches, n_items = _short(kind, rows)
    _assert_same(_run(monkeypatch, DEFAULT, "5in-b4", n_items, launches, dropout, loss, wd),
                 _run(monkeypatch, SCHED0, "5in-b4", n_items, launches, dropout, loss, wd))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_block5_lean2_biases_move_and_equal_sched0(shape, cuda, monkeypatch):
    """b0 and b2 are the packed pair of SCH_ADAM_B02: they and their moments leave their start values (b2 in
    every element, b0 in most units - one whose ReLU never fires has no gradient) and equal the previous
    schedule's."""
    dims, B = SHAPES[shape]
    launches = [63, 3]
    n_items = 66 * B - (1 if B > 1 else 0)
    new = _run(monkeypatch, DEFAULT, shape, n_items, launches, 0.2, "ce", 0.01)
    _assert_same(new, _run(monkeypatch, SCHED0, shape, n_items, launches, 0.2, "ce", 0.01))
    p0 = _data(shape)[3].cpu()
    sb0, sb2 = _bias_slices(dims)
    assert sb2.stop == p0.numel()
    assert bool((new[0][sb2] != p0[sb2]).all()) and bool((new[1][sb2] != 0).all()) and bool((new[2][sb2] != 0).all())
    moved = new[0][sb0] != p0[sb0]
    assert int(moved.sum()) > dims[1] // 2, int(moved.sum())
    assert int((new[1][sb0] != 0).sum()) > dims[1] // 2 and int((new[2][sb0] != 0).sum()) > dims[1] // 2


def test_block5_lean2_schedule_matches_lds_trainer_across_launches(cuda, monkeypatch):
    """Default schedule against the generic LDS trainer (same dropout hash, loss and Adam, another summation
    order) over the 63 + 3 launches with a short last batch, at the tolerance of tests/test_block5_sched_gpu.py."""
    opt = (0.2, "ce", 0.01)
    launches, n_items = [63, 3], 66 * 4 - 2
    new = _run(monkeypatch, DEFAULT, "5in-b4", n_items, launches, *opt)
    ref = _run(monkeypatch, dict(DEFAULT, DCT_MLP_KERNEL="lds", DCT_MLP_BLOCK="0"), "5in-b4", n_items, launches, *opt)
    for a_, b_ in zip(new, ref):
        assert torch.isfinite(a_).all()
        err = float((a_ - b_).abs().max())
        print(f"max|new - lds| = {err:.3e} (bound {1e-4 * (1 + float(b_.abs().max())):.3e})")
        assert err <= 1e-4 * (1 + b_.abs().max())
