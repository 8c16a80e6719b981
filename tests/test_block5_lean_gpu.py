"""Prefetch edges and dropout rates: mlp_block5's default step schedule against the previous schedule's own
instantiation (DCT_B5_SCHED=0, csrc/knobs.h), bit for bit: parameters, both Adam moments and every step's loss.
What this module guards (csrc/mlp_block5_impl.h): the next batch's gather only in wave 0, the small Adam pairs
packed in place, dZ2's ReLU / dropout factor published as floats, the dropout keep test on integers, db2 from a
quad sum.  Every value keeps its operation sequence.  Cases: the launch splits of
tests/test_block5_prio_defer_gpu.py over a data set whose batch order is a permutation of every row of X (seeds
31 / 17 / 3), and the prefetch's own edges: a dataset that ends with the last step (no next batch to fetch), one
of batch + 1 rows (the second batch has one row), an index order with the first and last row of X in the first
and last batches; dropout 0.5 and a rate whose integer threshold is 2 (1e-7).  The comparison with the LDS
trainer is in tests/test_block5_sched_gpu.py.  Helpers, splits and data sets: tests/block5_sched_cases.py."""
import pytest
import torch

import block5_sched_cases as bc
import dct_amd  # noqa: F401
from block5_sched_cases import CORNERS, DEFAULT, SHAPES, fresh_knobs  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu

CASES = bc.cases(["7x1", "2+1", "63+3", "40+30-short"], bc.OPTIONS)


@pytest.mark.parametrize("shape,split,dropout,loss,wd", CASES, ids=bc.ids(CASES))
def test_block5_lean_schedule_equals_sched0(shape, split, dropout, loss, wd, cuda, monkeypatch):
    bc.run_both(monkeypatch, DEFAULT, *bc.split_args(shape, split, 31, 17, spare=False), seed=3, dropout=dropout,
                loss=loss, wd=wd)


def _edge_args(shape, edge):
    """(dims, B, data, idx, launches) of a prefetch edge."""
    dims, B = SHAPES[shape]
    data = bc.shape_data(shape, 31, 17, spare=False)
    perm, N = data[2], data[0].shape[0]
    if edge == "ends-with-last-step":  # steps * B rows exactly: the last step has no next batch, one launch
        idx, steps = perm[:9 * B], [9]
    elif edge == "batch-plus-one-row":   # the second batch has one row
        idx, steps = perm[:B + 1], [2]
    elif edge == "one-row":              # a single step with a single row: nothing to prefetch at all
        idx, steps = perm[:1], [1]
    else:
        assert edge == "first-and-last-row"  # rows 0 and N - 1 of X in the first and in the last batch (batch 1:
        idx, steps = perm[:6 * B].clone(), [4, 2]  # in the first two and the last two)
        idx[0], idx[1], idx[-2], idx[-1] = 0, N - 1, N - 1, 0
    return dims, B, data, idx, bc.consecutive(steps)


EDGES = ["ends-with-last-step", "batch-plus-one-row", "one-row", "first-and-last-row"]
EDGE_CASES = [(shape, edge) + opt for shape in SHAPES for edge in EDGES for opt in CORNERS]


@pytest.mark.parametrize("shape,edge,dropout,loss,wd", EDGE_CASES, ids=bc.ids(EDGE_CASES))
def test_block5_lean_prefetch_edges_equal_sched0(shape, edge, dropout, loss, wd, cuda, monkeypatch):
    bc.run_both(monkeypatch, DEFAULT, *_edge_args(shape, edge), seed=3, dropout=dropout, loss=loss, wd=wd)


@pytest.mark.parametrize("dropout", [0.5, 1e-7], ids=["p0.5", "p1e-7"])
@pytest.mark.parametrize("shape", ["5in-b4", "8in-b3"])
def test_block5_lean_dropout_rates_equal_sched0(shape, dropout, cuda, monkeypatch):
    args = bc.split_args(shape, "63+3", 31, 17, spare=False)
    new = bc.run_both(monkeypatch, DEFAULT, *args, seed=3, dropout=dropout, loss="ce", wd=0.0)
    if dropout == 0.5:  # the rate does something: another trajectory than without dropout
        off = bc.run_launches(monkeypatch, DEFAULT, *args, seed=3, dropout=0.0, loss="ce", wd=0.0)
        assert not torch.equal(new[0], off[0])
