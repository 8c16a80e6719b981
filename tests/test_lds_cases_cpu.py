"""tests/lds_cases.py against the plan (csrc/mlp_fused.hip mlp_make_shape through ``MlpPlan``): every row is
supported, lands in the ownership class it names and reaches the generic LDS trainer, and the table covers all
42 instantiations of ``mlp_train_kernel``.  No GPU."""
import pytest

import dct_amd  # noqa: F401
from dct_amd.ops import _native
from dct_amd.ops.fused_mlp import FusedMLPKernel

import lds_cases

LDS_BUDGET = 160 * 1024


@pytest.fixture
def nat(monkeypatch):
    for k, v in lds_cases.ENV.items():
        monkeypatch.setenv(k, v)
    n = _native.native()
    yield n
    monkeypatch.undo()
    n.reload_knobs()


def _check(nat, dims, bmax, cls, batches):
    plan = nat.MlpPlan(dims, bmax)  # the constructor re-reads the knobs
    assert plan.supported
    assert (plan.threads, plan.max_blocks_per_thread, plan.block_rows) == cls
    for B in batches:
        assert plan.trainer(B, mode=0) == plan.trainer(B, mode=1) == "lds"
    return plan


@pytest.mark.parametrize("bmax", lds_cases.BMAXES)
@pytest.mark.parametrize("dims,cls", lds_cases.TABLE, ids=[lds_cases.name(d) for d, _ in lds_cases.TABLE])
def test_row_lands_in_its_class(dims, cls, bmax, nat):
    _check(nat, dims, bmax, cls, (bmax, 1) if bmax == 4 else (16, 9))


def test_table_covers_all_42_instantiations():
    got = {(len(dims) - 1, bmax, cls) for dims, bmax, cls in lds_cases.kernels()}
    want = {(L, bmax, cls) for L in (2, 3, 4) for bmax in lds_cases.BMAXES for cls in lds_cases.CLASSES}
    assert len(got) == 42 and got == want
    assert len(lds_cases.smallest_per_class()) == 7


@pytest.mark.parametrize("dims,bmaxes,cls,batch,what", lds_cases.EDGES,
                         ids=[lds_cases.name(e[0]) for e in lds_cases.EDGES])
def test_edge_rows_sit_on_their_edges(dims, bmaxes, cls, batch, what, nat):
    for bmax in bmaxes:
        plan = _check(nat, dims, bmax, cls, (batch or bmax,))
        assert plan.lds_bytes <= LDS_BUDGET
        if tuple(dims) in lds_cases.EDGE_LDS_BYTES:
            assert plan.lds_bytes == lds_cases.EDGE_LDS_BYTES[tuple(dims)]
        if "nbias" in what:
            assert sum(dims[1:]) == 2 * plan.threads
            assert not nat.MlpPlan(dims[:1] + [dims[1] + 1] + dims[2:], bmax).supported  # one more bias: refused
        if batch is not None:  # the prefetch switch pf = (B * D0 + B <= threads) of mlp_train_kernel
            fits = batch * dims[0] + batch <= plan.threads
            assert fits == ("prefetch" in what)
            assert (batch * dims[0] + batch == plan.threads) == ("exact fit" in what)


VALIDATE_EDGE = [([21, 164, 164, 5], 144128, 178880), ([14, 116, 116, 116, 5], 134032, 169936)]


@pytest.mark.parametrize("dims,bytes4,bytes16", VALIDATE_EDGE, ids=[lds_cases.name(d) for d, _, _ in VALIDATE_EDGE])
def test_shapes_supported_at_batch_4_only_have_an_evaluation_plan(dims, bytes4, bytes16, nat):
    """Their 16-row layout overflows the LDS budget: ``supported`` accepts them at batch <= 4, so the
    evaluation falls back to 4-row chunks (tests/test_lds_trainer_gpu.py runs it)."""
    assert FusedMLPKernel.supported(dims, 4) and not FusedMLPKernel.supported(dims, 16)
    assert nat.MlpPlan(dims, 4).lds_bytes == bytes4 and nat.MlpPlan(dims, 16).lds_bytes == bytes16
    assert bytes4 <= LDS_BUDGET < bytes16
    k = FusedMLPKernel(dims, bmax=4)
    assert k.eval_plan.bmax == 4 and k.eval_plan.eval_fits
    # every other shape keeps the 16-row evaluation
    assert FusedMLPKernel([5, 128, 128, 2], bmax=4).eval_plan.bmax == 16


def test_fp32_reference_keeps_sqrt_v_within_a_quarter_of_the_bound_on_m(monkeypatch):
    """Where tests/test_lds_trainer_gpu.py's sqrt(v) bound comes from: the plain fp32 torch reference of each of
    its trajectory cases, under the same masks, against the fp64 one (6.2e-4 of m's bound at worst when
    measured).  Under a quarter, the GPU tests hold sqrt(v) to m's bound itself."""
    import test_lds_trainer_gpu as T

    cases = [(d, B, loss, 0.0, 0) for d, _, B in T.TRAJECTORIES for loss in T.LOSSES]
    cases += [(d, B, loss, T.WEIGHT_DECAY, 0) for d, _, B in T.DECAYED for loss in T.LOSSES]
    cases += [(T.COUNTER_CASE[0], T.COUNTER_CASE[2], "ce", 0.0, 9)]
    worst = max(T.fp32_reference_sqrt_v_ratio(d, B, loss, wd, monkeypatch, first_gstep=g0)
                for d, B, loss, wd, g0 in cases)
    print("worst fp32-reference ratio %.2e" % worst)
    assert worst < T.FP32_RATIO_LIMIT and T.SQRT_V_BOUND == 1.0
    _native.native().reload_knobs()


def test_every_supported_shape_has_an_evaluation_plan(nat):
    """``supported`` never promises a model ``evaluate`` refuses: over a sweep of widths around the LDS
    budget, whatever trains at some batch limit has an evaluation plan that fits."""
    for L, widths in ((2, range(150, 700, 37)), (3, range(100, 200, 7)), (4, range(90, 140, 5))):
        for h in widths:
            for d0 in (3, 30):
                dims = [d0] + [h] * (L - 1) + [5]
                for batch in (4, 16):
                    if FusedMLPKernel.supported(dims, batch):
                        assert FusedMLPKernel(dims, bmax=batch).eval_plan.eval_fits, (dims, batch)
    tiled = 0  # the batch-tiled trainer's shapes (batch 17 .. 1024) validate through the same kernel
    for dims in ([32, 128, 4], [32, 128, 128, 4], [5, 128, 128, 2], [7, 48, 32, 3], [1, 16, 1]):
        if FusedMLPKernel.supported(dims, 17):
            tiled += 1
            assert FusedMLPKernel(dims, bmax=1024).eval_plan.eval_fits, dims
    assert tiled >= 3
