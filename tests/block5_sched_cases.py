"""What the tests/test_block5_*_gpu.py modules of the step schedule share: mlp_block5's default step schedule
against the previous schedule's own instantiation (DCT_B5_SCHED=0, csrc/knobs.h) and against the generic LDS
trainer.

The knob-reload fixture, shapes, launch splits and option sets, start parameters, data sets, the launch runner,
the two comparisons and the environments of the kernels compared.  A plain module, not a conftest: the test
modules import it."""
import functools
import math

import pytest
import torch

from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import FusedMLPKernel

# (dims, batch): the headline shape, the widest input at a batch below the quad's four rows, the narrowest at batch 1
SHAPES = {"5in-b4": ([5, 128, 128, 2], 4),
          "8in-b3": ([8, 128, 128, 2], 3),
          "1in-b1": ([1, 128, 128, 2], 1)}

MAX_STEPS = 70
# steps of each launch, rows missing in the last batch (batch 1 has none to miss)
SPLITS = {"7x1": ([1] * 7, 0),  # every step is a launch's first and last
          "2+1": ([2, 1], 0),
          "63+3": ([63, 3], 0),  # the second launch straddles the 64-step block of the Adam-scalar table
          "40+30": ([40, 30], 0),
          "40+30-short": ([40, 30], 1)}
# (dropout, loss, weight decay): the whole cross on the headline shape, two opposite corners on the others
OPTIONS = [(d, l, w) for d in (0.0, 0.2) for l in ("ce", "mse") for w in (0.0, 0.01)]
OPTIONS_P05 = [(d, l, w) for d in (0.0, 0.2, 0.5) for l in ("ce", "mse") for w in (0.0, 0.01)]
CORNERS = [(0.2, "ce", 0.01), (0.0, "mse", 0.0)]


def cases(splits, options):
    """(shape, split, dropout, loss, wd): options on the headline shape, CORNERS on the others."""
    return [(shape, split) + opt for shape in SHAPES for split in splits
            for opt in (options if shape == "5in-b4" else CORNERS)]


def ids(cs):
    return ["-".join(str(x) for x in c) for c in cs]


def split_items(shape, split):
    """(step counts, dataset size) of a split."""
    steps, short = SPLITS[split]
    B = SHAPES[shape][1]
    return steps, sum(steps) * B - min(short, B - 1)


# a value of None: unset
DEFAULT = {"DCT_B5_SCHED": None, "DCT_MLP_KERNEL": None, "DCT_MLP_BLOCK": None}
SCHED1 = dict(DEFAULT, DCT_B5_SCHED="1")  # the default schedule, named
SCHED0 = dict(DEFAULT, DCT_B5_SCHED="0")  # the previous schedule
LDS = dict(DEFAULT, DCT_MLP_KERNEL="lds", DCT_MLP_BLOCK="0")  # no wave kernel, no 3x128 block kernel


@pytest.fixture(autouse=True)
def fresh_knobs():
    """Every test starts from the environment's knobs (a test module imports the fixture to use it)."""
    native().reload_knobs()


def flat_params(dims, seed):
    g = torch.Generator().manual_seed(seed)
    parts = []
    for i in range(len(dims) - 1):
        bound = 1.0 / math.sqrt(dims[i])
        parts.append((torch.rand(dims[i + 1], dims[i], generator=g) * 2 - 1) * bound)
        parts.append((torch.rand(dims[i + 1], generator=g) * 2 - 1) * bound)
    return torch.cat([t.reshape(-1) for t in parts])


@functools.lru_cache(maxsize=None)
def data(dims, data_seed, param_seed, n_rows, n_idx):
    """(X, Y, idx, p0) on the GPU (shared by the cases that name it, never written): n_rows inputs and
    labels, the first n_idx entries of a permutation of the rows as the batch order, start parameters.
    dims: a tuple."""
    g = torch.Generator().manual_seed(data_seed)
    X = torch.randn(n_rows, dims[0], generator=g).cuda()
    Y = torch.randint(0, dims[-1], (n_rows,), generator=g).to("cuda", torch.int32)
    idx = torch.randperm(n_rows, generator=g)[:n_idx].to("cuda", torch.int32)
    return X, Y, idx, flat_params(list(dims), param_seed).cuda()


def sized_data(dims, n_items, data_seed, param_seed):
    """A data set with spare rows, sized by the case: idx names n_items of its 2 * n_items + 7 rows."""
    return data(tuple(dims), data_seed, param_seed, 2 * n_items + 7, n_items)


def shape_data(shape, data_seed, param_seed, spare):
    """A shape's data set of MAX_STEPS batches; spare: as many rows again (+ 7) that idx does not name,
    otherwise idx is a permutation of every row."""
    dims, B = SHAPES[shape]
    n = MAX_STEPS * B
    return data(tuple(dims), data_seed, param_seed, 2 * n + 7 if spare else n, n)


def consecutive(steps):
    """Launches of the given step counts, each starting at the step count and dropout step the one before
    it reached: [(first step, steps, t0, step_base)]."""
    out, first = [], 0
    for n in steps:
        out.append((first, n, first, first))
        first += n
    return out


def rows_args(shape, n_items, steps, data_seed, param_seed, spare):
    """(dims, B, data, idx, launches) for run_launches / run_both: launches of the given step counts over the first
    n_items rows of the batch order of shape_data(shape, data_seed, param_seed, spare)."""
    dims, B = SHAPES[shape]
    d = shape_data(shape, data_seed, param_seed, spare)
    return dims, B, d, d[2][:n_items], consecutive(steps)


def split_args(shape, split, data_seed, param_seed, spare):
    """rows_args of a split of SPLITS."""
    steps, n_items = split_items(shape, split)
    return rows_args(shape, n_items, steps, data_seed, param_seed, spare)


def run_launches(monkeypatch, env, dims, B, data, idx, launches, *, seed, dropout, loss, wd):
    """launches ([(first step, steps, t0, step_base)], consecutive) over the rows idx names (its length is the
    dataset's size) under env; returns (p, m, v, losses) on the CPU."""
    for k_, v_ in env.items():
        if v_ is None:
            monkeypatch.delenv(k_, raising=False)
        else:
            monkeypatch.setenv(k_, v_)
    X, Y, _, p0 = data
    n_items = int(idx.numel())
    steps = math.ceil(n_items / B)
    assert sum(n for _, n, _, _ in launches) == steps
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    losses = torch.zeros(steps, device=p0.device)
    k = FusedMLPKernel(dims, bmax=4)  # (re-reads the knobs)
    assert k.plan.trainer(B) == ("lds" if env.get("DCT_MLP_BLOCK") == "0" else "block5")  # the kernel under test
    for first, n, t0, sbase in launches:
        k.train(p, m, v, X, Y, idx[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=t0, lr=0.01,
                weight_decay=wd, dropout=dropout, seed=seed, step_base=sbase, loss=loss, loss_out=losses[first:])
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu(), losses.cpu()


def assert_same(new, old):
    for name, a_, b_ in zip("pmvl", new, old):
        assert torch.isfinite(a_).all(), name
        assert torch.equal(a_, b_), (name, float((a_ - b_).abs().max()))
    assert bool((new[3] != 0).all())  # every step of every launch wrote its loss


def run_both(monkeypatch, env, dims, B, data, idx, launches, **opt):
    """The launches under env and under DCT_B5_SCHED=0, compared bit for bit; returns env's result."""
    new = run_launches(monkeypatch, env, dims, B, data, idx, launches, **opt)
    assert_same(new, run_launches(monkeypatch, SCHED0, dims, B, data, idx, launches, **opt))
    return new


def assert_close_to_lds(new, ref):
    """The generic LDS trainer is an independent kernel: same dropout hash, loss and Adam, another summation
    order."""
    for a_, b_ in zip(new, ref):
        assert torch.isfinite(a_).all()
        err = float((a_ - b_).abs().max())
        print(f"max|new - lds| = {err:.3e} (bound {1e-4 * (1 + float(b_.abs().max())):.3e})")
        assert err <= 1e-4 * (1 + b_.abs().max())
