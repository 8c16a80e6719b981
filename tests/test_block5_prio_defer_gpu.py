"""Launch boundaries: mlp_block5's default step schedule against the previous schedule's own instantiation
(DCT_B5_SCHED=0, csrc/knobs.h), bit for bit: parameters, moments and per-step losses.  The cases were set for the
W2 / b1 / b2 owners' Adam of step s deferred into step s + 1, in front of barrier A: it carried that step's
gradient sums and Adam scalars, was skipped in a launch's first step and flushed after its last one.  It measured
slower and was removed; the cases stay, since what a schedule item that carries state
across steps gets wrong is launch boundaries and the carried scalars: launches of one step (every step first and
last), 2 + 1, 63 + 3 (the second launch straddles the 64-step block of the Adam-scalar table) and 40 + 30 with a
short last batch.  Data set: spare rows, seeds 29 / 13 / 3; its comparison with the LDS trainer is in
tests/test_block5_sched_gpu.py.  Helpers, splits and data sets: tests/block5_sched_cases.py."""
import pytest

import block5_sched_cases as bc
import dct_amd  # noqa: F401
from block5_sched_cases import DEFAULT, fresh_knobs  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu

CASES = bc.cases(["7x1", "2+1", "63+3", "40+30-short"], bc.OPTIONS)


@pytest.mark.parametrize("shape,split,dropout,loss,wd", CASES, ids=bc.ids(CASES))
def test_block5_default_schedule_equals_sched0_at_launch_boundaries(shape, split, dropout, loss, wd, cuda, monkeypatch):
    bc.run_both(monkeypatch, DEFAULT, *bc.split_args(shape, split, 29, 13, spare=True), seed=3, dropout=dropout,
                loss=loss, wd=wd)
