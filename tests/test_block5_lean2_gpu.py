"""Short last batches and the bias pair: mlp_block5's default step schedule against the previous schedule's own
instantiation (DCT_B5_SCHED=0, csrc/knobs.h), bit for bit: parameters, both Adam moments and every step's loss.
What this module guards (csrc/mlp_block5_impl.h): the logit shares as a reduce-scatter, 1 / bs once per launch
with the per-step form behind a scalar branch for a short batch, b0 and b2 as one packed Adam pair updated at
the dW0 / db0 tail (b2 published there).  Every value keeps its operation sequence.  Cases: three shapes, the
launch splits of tests/test_block5_lean_gpu.py with full batches, last batches of 1, 2 and 3 rows at batch 4 -
inside a multi-step launch, as a dataset of that batch alone (one one-step launch) and as the first step of a
launch that follows a full one -, cross-entropy and MSE, weight decay 0 and 0.01, dropout 0, 0.2 and 0.5.  One
case also checks that b0 and b2 moved from their start values, so the comparison cannot pass on parameters
nothing touched.  Data set: idx a permutation of every row, seeds 43 / 23 / 5; its comparison with the LDS
trainer is in tests/test_block5_sched_gpu.py.  Helpers, splits and data sets: tests/block5_sched_cases.py."""
import pytest

import block5_sched_cases as bc
import dct_amd  # noqa: F401
from block5_sched_cases import CORNERS, DEFAULT, SHAPES, fresh_knobs  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu

CASES = bc.cases(["7x1", "2+1", "63+3", "40+30"], bc.OPTIONS_P05)


@pytest.mark.parametrize("shape,split,dropout,loss,wd", CASES, ids=bc.ids(CASES))
def test_block5_lean2_schedule_equals_sched0(shape, split, dropout, loss, wd, cuda, monkeypatch):
    bc.run_both(monkeypatch, DEFAULT, *bc.split_args(shape, split, 43, 23, spare=False), seed=5, dropout=dropout,
                loss=loss, wd=wd)


# last batches of 1, 2 and 3 rows at batch 4: (step counts, rows of the dataset)
def _short(kind, rows):
    if kind == "in-launch":        # the last step of a 30-step launch
        return [40, 30], 69 * 4 + rows
    if kind == "only-batch":       # the dataset is the short batch: one one-step launch
        return [1], rows
    assert kind == "first-step"    # a launch of full batches, then one that starts with the short batch
    return [6, 1], 6 * 4 + rows


SHORT_CASES = [(kind, rows) + opt for kind in ("in-launch", "only-batch", "first-step") for rows in (1, 2, 3)
               for opt in CORNERS + [(0.5, "ce", 0.0)]]


@pytest.mark.parametrize("kind,rows,dropout,loss,wd", SHORT_CASES, ids=bc.ids(SHORT_CASES))
def test_block5_lean2_short_last_batch_equals_sched0(kind, rows, dropout, loss, wd, cuda, monkeypatch):
    steps, n_items = _short(kind, rows)
    bc.run_both(monkeypatch, DEFAULT, *bc.rows_args("5in-b4", n_items, steps, 43, 23, spare=False), seed=5,
                dropout=dropout, loss=loss, wd=wd)


def _bias_slices(dims):
    """Flat-parameter slices of b0 and b2 (torch order: W0, b0, W1, b1, W2, b2)."""
    b0 = dims[1] * dims[0]
    b2 = b0 + dims[1] + dims[2] * dims[1] + dims[2] + dims[3] * dims[2]
    return slice(b0, b0 + dims[1]), slice(b2, b2 + dims[3])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_block5_lean2_biases_move_and_equal_sched0(shape, cuda, monkeypatch):
    """b0 and b2 are one packed Adam pair in the schedule: they and their moments leave their start values (b2
    in every element, b0 in most units - one whose ReLU never fires has no gradient) and equal the previous
    schedule's."""
    dims, B = SHAPES[shape]
    n_items = 66 * B - (1 if B > 1 else 0)
    args = bc.rows_args(shape, n_items, [63, 3], 43, 23, spare=False)
    new = bc.run_both(monkeypatch, DEFAULT, *args, seed=5, dropout=0.2, loss="ce", wd=0.01)
    p0 = args[2][3].cpu()
    sb0, sb2 = _bias_slices(dims)
    assert sb2.stop == p0.numel()
    assert bool((new[0][sb2] != p0[sb2]).all()) and bool((new[1][sb2] != 0).all()) and bool((new[2][sb2] != 0).all())
    moved = new[0][sb0] != p0[sb0]
    assert int(moved.sum()) > dims[1] // 2, int(moved.sum())
    assert int((new[1][sb0] != 0).sum()) > dims[1] // 2 and int((new[2][sb0] != 0).sum()) > dims[1] // 2
