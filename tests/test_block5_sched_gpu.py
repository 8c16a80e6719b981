"""mlp_block5's default step schedule against the previous schedule's own instantiation (DCT_B5_SCHED=0,
csrc/knobs.h), bit for bit: parameters, both Adam moments and every step's loss.  The schedule
(csrc/mlp_block5_impl.h) moves gradient-free work of the step out of the contended backward and takes vector
instructions the result does not need out of the loop; every value keeps its operation sequence.  This module:
  * the Adam-scalar table (64 steps per refresh) and launches that start inside a block of it;
  * shapes: one, five and eight inputs at batch 1, 4 and 3.  The 70-step cases were set for an interleaved
    dZ1 / dW1 / Adam backward that measured slower and was removed;
  * the generic LDS trainer, the independent reference that keeps the knob from selecting nothing, over the
    data set of each of the schedule's test modules.
Launch boundaries: tests/test_block5_prio_defer_gpu.py; prefetch edges and dropout rates:
tests/test_block5_lean_gpu.py; short last batches and the bias pair: tests/test_block5_lean2_gpu.py.
Helpers, data sets and environments: tests/block5_sched_cases.py."""
import math

import pytest

import block5_sched_cases as bc
import dct_amd  # noqa: F401
from block5_sched_cases import DEFAULT, LDS, SCHED1, SHAPES, fresh_knobs  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu


# ---- Adam-scalar table and launch starts -----------------------------------------------------------------
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
    data = bc.sized_data(dims, n_items, 17, 5)
    bc.run_both(monkeypatch, SCHED1, dims, B, data, data[2], launches, seed=3, dropout=dropout, loss=loss, wd=wd)


# ---- shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,B,n_items", [([8, 128, 128, 2], 3, 200), ([1, 128, 128, 2], 1, 70)])
@pytest.mark.parametrize("split", [True, False], ids=["two-launches", "t0-3-base-5"])
def test_block5_schedule_equals_previous_other_shapes(dims, B, n_items, split, cuda, monkeypatch):
    """Eight inputs at batch 3 (67 steps, the last with 2 rows) and one input at batch 1 (70 steps)."""
    steps = math.ceil(n_items / B)
    launches = [(0, 40, 0, 0), (40, steps - 40, 40, 40)] if split else [(0, steps, 3, 5)]
    data = bc.sized_data(dims, n_items, 17, 5)
    bc.run_both(monkeypatch, SCHED1, dims, B, data, data[2], launches, seed=3, dropout=0.2, loss="ce", wd=0.01)


# 70 steps in two launches of 40 + 30; the last step of the first two shapes is one row short
ITEMS_70 = {"5in-b4": 69 * 4 + 3, "8in-b3": 69 * 3 + 2, "1in-b1": 70}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dropout", [0.0, 0.2])
def test_block5_default_schedule_equals_sched0_bitwise(dropout, loss, wd, shape, cuda, monkeypatch):
    dims, B = SHAPES[shape]
    data = bc.sized_data(dims, ITEMS_70[shape], 23, 11)
    bc.run_both(monkeypatch, DEFAULT, dims, B, data, data[2], bc.consecutive([40, 30]), seed=3, dropout=dropout,
                loss=loss, wd=wd)


# ---- the LDS-trainer reference -----------------------------------------------------------------------------
def _against_lds(monkeypatch, args, **opt):
    bc.assert_close_to_lds(bc.run_launches(monkeypatch, DEFAULT, *args, **opt),
                           bc.run_launches(monkeypatch, LDS, *args, **opt))


def test_block5_schedule_matches_lds_trainer(cuda, monkeypatch):
    """Over the 131 steps in one launch."""
    dims, B, n_items = [5, 128, 128, 2], 4, 523
    data = bc.sized_data(dims, n_items, 17, 5)
    opt = dict(seed=3, dropout=0.2, loss="ce", wd=0.0)
    bc.assert_close_to_lds(bc.run_launches(monkeypatch, SCHED1, dims, B, data, data[2], ONE, **opt),
                           bc.run_launches(monkeypatch, LDS, dims, B, data, data[2], ONE, **opt))


def test_block5_default_schedule_matches_lds_trainer(cuda, monkeypatch):
    """Over 40 + 30 steps, the last one a row short."""
    dims, B = SHAPES["5in-b4"]
    data = bc.sized_data(dims, ITEMS_70["5in-b4"], 23, 11)
    _against_lds(monkeypatch, (dims, B, data, data[2], bc.consecutive([40, 30])), seed=3, dropout=0.2, loss="ce",
                 wd=0.01)


def test_block5_default_schedule_matches_lds_trainer_across_launches(cuda, monkeypatch):
    """Over the 63 + 3 launches, the data set of tests/test_block5_prio_defer_gpu.py."""
    _against_lds(monkeypatch, bc.split_args("5in-b4", "63+3", 29, 13, spare=True), seed=3, dropout=0.2, loss="ce",
                 wd=0.01)


def test_block5_lean_schedule_matches_lds_trainer_across_launches(cuda, monkeypatch):
    """Over the 63 + 3 launches, the data set of tests/test_block5_lean_gpu.py (idx a permutation of every row)."""
    _against_lds(monkeypatch, bc.split_args("5in-b4", "63+3", 31, 17, spare=False), seed=3, dropout=0.2, loss="ce",
                 wd=0.01)


def test_block5_lean2_schedule_matches_lds_trainer_across_launches(cuda, monkeypatch):
    """Over the 63 + 3 launches with a short last batch, the data set of tests/test_block5_lean2_gpu.py."""
    _against_lds(monkeypatch, bc.rows_args("5in-b4", 66 * 4 - 2, [63, 3], 43, 23, spare=False), seed=5, dropout=0.2,
                 loss="ce", wd=0.01)
