"""mlp_block5's default step schedule against the previous schedule's own instantiation (DCT_B5_SCHED=0,
csrc/knobs.h), bit for bit: parameters, both Adam moments and every step's loss.  Round 11's items take
vector instructions the result does not need out of the step loop (csrc/mlp_block5_impl.h, SCH_PF_W0 ..
SCH_DB2): the next batch's gather only in wave 0, the small Adam pairs packed in place, dZ2's ReLU / dropout
factor published as floats, the dropout keep test on integers, db2 from a quad sum.  Every value keeps its
operation sequence.  Cases: the launch splits of tests/test_block5_prio_defer_gpu.py (one-step launches,
2 + 1, 63 + 3 across the Adam-scalar table's 64-step block, 40 + 30 with a short last batch), and the
prefetch's own edges: a dataset that ends with the last step (no next batch to fetch), one of batch + 1
rows (the second batch has one row), an index order with the first and last row of X in the first and last
batches; dropout 0.5 and a rate whose integer threshold is 2 (1e-7).  The generic LDS trainer is the
independent reference that keeps the knob from selecting nothing."""
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
    """Inputs, labels, batch order and start parameters of one shape (shared by its cases, never written).
    X has exactly MAX_STEPS * B rows and idx is a permutation of all of them."""
    dims, B = SHAPES[shape]
    g = torch.Generator().manual_seed(31)
    N = MAX_STEPS * B
    X = torch.randn(N, dims[0], generator=g).cuda()
    Y = torch.randint(0, dims[-1], (N,), generator=g).to("cuda", torch.int32)
    idx = torch.randperm(N, generator=g).to("cuda", torch.int32)
    return X, Y, idx, _flat_params(dims, 17).cuda()


def _run(monkeypatch, env, shape, idx, launches, dropout, loss, wd):
    """The launches over the rows idx names (its length is the dataset's size) under env (a value of None:
    unset); returns (p, m, v, losses) on the CPU."""
    for k_, v_ in env.items():
        if v_ is None:
            monkeypatch.delenv(k_, raising=False)
        else:
            monkeypatch.setenv(k_, v_)
    dims, B = SHAPES[shape]
    steps, n_items = sum(launches), int(idx.numel())
    assert math.ceil(n_items / B) == steps <= MAX_STEPS
    X, Y, _, p0 = _data(shape)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    losses = torch.zeros(steps, device=p0.device)
    k = FusedMLPKernel(dims, bmax=4)  # (re-reads the knobs)
    assert k.plan.trainer(B) == ("lds" if env.get("DCT_MLP_BLOCK") == "0" else "block5")  # the kernel under test
    first = 0
    for n in launches:
        k.train(p, m, v, X, Y, idx[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=first, lr=0.01,
                weight_decay=wd, dropout=dropout, seed=3, step_base=first, loss=loss, loss_out=losses[first:])
        first += n
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu(), losses.cpu()


def _split_idx(shape, split):
    dims, B = SHAPES[shape]
    launches, short = SPLITS[split]
    n_items = sum(launches) * B - min(short, B - 1)
    return _data(shape)[2][:n_items], launches


DEFAULT = {"DCT_B5_SCHED": None, "DCT_MLP_KERNEL": None, "DCT_MLP_BLOCK": None}
SCHED0 = dict(DEFAULT, DCT_B5_SCHED="0")


def _assert_same(new, old):
    for name, a_, b_ in zip("pmvl", new, old):
        assert torch.isfinite(a_).all(), name
        assert torch.equal(a_, b_), (name, float((a_ - b_).abs().max()))
    assert bool((new[3] != 0).all())  # every step of every launch wrote its loss


@pytest.mark.parametrize("shape,split,dropout,loss,wd", CASES,
                         ids=["-".join(str(x) for x in c) for c in CASES])
def test_block5_lean_schedule_equals_sched0(shape, split, dropout, loss, wd, cuda, monkeypatch):
    idx, launches = _split_idx(shape, split)
    _assert_same(_run(monkeypatch, DEFAULT, shape, idx, launches, dropout, loss, wd),
                 _run(monkeypatch, SCHED0, shape, idx, launches, dropout, loss, wd))


def _edge_idx(shape, edge):
    """(idx, launches) of a prefetch edge."""
    dims, B = SHAPES[shape]
    X, _, perm, _ = _data(shape)
    N = X.shape[0]
    if edge == "ends-with-last-step":  # steps * B rows exactly: the last step has no next batch, one launch
        return perm[:9 * B], [9]
    if edge == "batch-plus-one-row":   # the second batch has one row
        return perm[:B + 1], [2]
    if edge == "one-row":              # a single step with a single row: nothing to prefetch at all
        return perm[:1], [1]
    assert edge == "first-and-last-row"  # rows 0 and N - 1 of X in the first and in the last batch (batch 1:
    idx = perm[:6 * B].clone()           # in the first two and the last two)
    idx[0], idx[1], idx[-2], idx[-1] = 0, N - 1, N - 1, 0
    return idx, [4, 2]


EDGES = ["ends-with-last-step", "batch-plus-one-row", "one-row", "first-and-last-row"]
EDGE_CASES = [(shape, edge) + opt for shape in SHAPES for edge in EDGES for opt in CORNERS]


@pytest.mark.parametrize("shape,edge,dropout,loss,wd", EDGE_CASES,
                         ids=["-".join(str(x) for x in c) for c in EDGE_CASES])
def test_block5_lean_prefetch_edges_equal_sched0(shape, edge, dropout, loss, wd, cuda, monkeypatch):
    idx, launches = _edge_idx(shape, edge)
    _assert_same(_run(monkeypatch, DEFAULT, shape, idx, launches, dropout, loss, wd),
                 _run(monkeypatch, SCHED0, shape, idx, launches, dropout, loss, wd))


@pytest.mark.parametrize("dropout", [0.5, 1e-7], ids=["p0.5", "p1e-7"])
@pytest.mark.parametrize("shape", ["5in-b4", "8in-b3"])
def test_block5_lean_dropout_rates_equal_sched0(shape, dropout, cuda, monkeypatch):
    idx, launches = _split_idx(shape, "63+3")
    new = _run(monkeypatch, DEFAULT, shape, idx, launches, dropout, "ce", 0.0)
    _assert_same(new, _run(monkeypatch, SCHED0, shape, idx, launches, dropout, "ce", 0.0))
    if dropout == 0.5:  # the rate does something: another trajectory than without dropout
        off = _run(monkeypatch, DEFAULT, shape, idx, launches, 0.0, "ce", 0.0)
        assert not torch.equal(new[0], off[0])


def test_block5_lean_schedule_matches_lds_trainer_across_launches(cuda, monkeypatch):
    """Default schedule against the generic LDS trainer (same dropout hash, loss and Adam, another summation
    order) over the 63 + 3 launches, at the tolerance of tests/test_block5_sched_gpu.py."""
    idx, launches = _split_idx("5in-b4", "63+3")
    opt = (0.2, "ce", 0.01)
    new = _run(monkeypatch, DEFAULT, "5in-b4", idx, launches, *opt)
    ref = _run(monkeypatch, dict(DEFAULT, DCT_MLP_KERNEL="lds", DCT_MLP_BLOCK="0"), "5in-b4", idx, launches, *opt)
    for a_, b_ in zip(new, ref):
        assert torch.isfinite(a_).all()
        err = float((a_ - b_).abs().max())
        print(f"max|new - lds| = {err:.3e} (bound {1e-4 * (1 + float(b_.abs().max())):.3e})")
        assert err <= 1e-4 * (1 + b_.abs().max())
