"""Which trainer a small-MLP launch reaches (csrc/mlp_select.cpp through ``MlpPlan.trainer``): one table of
(dims, plan bmax, environment, launch description) -> trainer name.  No GPU.

Every expected name was derived by hand from the dispatch as it stood before the selector existed
(MlpPlan's constructor, launch_train, dct_mlp_wave_train / rows_eligible, dct_mlp_train with
mlp_block5_ok / mlp_block3_ok, mlp_launch_block5); each row's comment names the clause that decides it.
The GPU tests that pin a kernel assert the same names next to their launches."""
import pytest

import dct_amd  # noqa: F401
from dct_amd.ops import _native

AUTO, LDS, BLOCK0, BLOCK3, BLOCK8, TILE = ({}, {"DCT_MLP_KERNEL": "lds"}, {"DCT_MLP_BLOCK": "0"},
                                           {"DCT_MLP_BLOCK": "3"}, {"DCT_MLP_BLOCK": "8"}, {"DCT_MLP_BLOCK": "tile"})
# tests/test_kernels_gpu.py's KERNELS, in its order: auto, lds, lds-noblock, lds-b3
KERNEL_ENVS = [{"DCT_MLP_KERNEL": "auto", "DCT_MLP_BLOCK": "-1"}, {"DCT_MLP_KERNEL": "lds", "DCT_MLP_BLOCK": "-1"},
               {"DCT_MLP_KERNEL": "lds", "DCT_MLP_BLOCK": "0"}, {"DCT_MLP_KERNEL": "lds", "DCT_MLP_BLOCK": "3"}]
W3 = [5, 128, 128, 2]  # the weather 3x128 net
GRAD, TRAIN = dict(mode=1), dict(mode=0)


def _bmax(B):
    return 4 if B <= 4 else (16 if B <= 16 else 1024)


def _row(dims, B, env, query, want, bmax=None):
    return (dims, bmax or _bmax(B), env, dict(query, batch=B), want)


TABLE = []

# ---- tests/test_dropout_reference_gpu.py, grad mode
for dims, B in [([5, 64, 2], 4), ([5, 64, 2], 3), ([7, 20, 2], 8), ([16, 64, 4], 5), ([9, 48, 64, 3], 4),
                ([9, 48, 64, 3], 8), ([12, 40, 40, 4], 6)]:
    TABLE.append(_row(dims, B, AUTO, GRAD, "wave_single"))  # wave plan, batch <= 8; rows_eligible wants train mode
TABLE += [
    _row([5, 64, 2], 16, AUTO, GRAD, "lds"),  # dct_mlp_wave_supported: batch > 8
    _row([7, 20, 2], 9, AUTO, GRAD, "lds"),  # the same
    _row([12, 40, 4], 6, LDS, GRAD, "lds"),  # DCT_MLP_KERNEL=lds clears use_wave; no 3x128 shape
    _row([16, 32, 48, 32, 3], 16, AUTO, GRAD, "lds"),  # 4 layers: neither wave nor block
    _row(W3, 4, BLOCK0, GRAD, "lds"),  # DCT_MLP_BLOCK=0 skips block5 and block3
    _row([7, 128, 128, 2], 4, BLOCK3, GRAD, "block3"),  # DCT_MLP_BLOCK=3 skips block5
    _row([30, 128, 128, 3], 3, BLOCK3, GRAD, "block3"),
]
for dims, B in [(W3, 4), (W3, 3), ([8, 128, 128, 2], 1), ([1, 128, 128, 2], 2)]:
    TABLE.append(_row(dims, B, AUTO, GRAD, "block5"))  # mlp_block5_ok: D0 <= 8, 2 classes, one-step grad mode
for dims, B in [(W3, 8), ([3, 128, 128, 2], 7)]:
    TABLE.append(_row(dims, B, AUTO, GRAD, "block5_b8"))  # mlp_launch_block5: batch > 4
for dims, B in [([5, 64, 2], 17), (W3, 33), (W3, 100), ([7, 48, 32, 3], 65), ([7, 32, 48, 3], 40),
                ([32, 128, 128, 4], 17)]:
    TABLE.append(_row(dims, B, AUTO, GRAD, "tile"))  # bmax 1024 forces the tile plan
# ---- tests/test_dropout_reference_gpu.py, train mode and trajectories
for dims, B in [([5, 64, 2], 4), ([5, 64, 2], 8), ([5, 64, 2], 3), ([8, 48, 3], 5), ([16, 64, 4], 2)]:
    TABLE.append(_row(dims, B, AUTO, TRAIN, "wave_rows"))  # rows_eligible: 2 layers, train mode, m and v bound
TABLE += [
    _row(W3, 4, AUTO, TRAIN, "block5"),
    _row(W3, 8, AUTO, TRAIN, "block5_b8"),
    _row(W3, 4, BLOCK3, TRAIN, "block3"),
    _row([5, 64, 2], 16, AUTO, TRAIN, "lds"),
    _row(W3, 33, AUTO, TRAIN, "tile"),
    _row([9, 48, 64, 3], 4, AUTO, TRAIN, "wave_single"),  # rows_eligible: L == 2 only
]
# ---- tests/test_kernels_gpu.py: test_fused_train_matches_torch_adam's shapes x KERNELS
WAVE2 = ("wave_rows", "lds", "lds", "lds")  # DCT_MLP_KERNEL=lds clears use_wave
ALL_LDS = ("lds",) * 4
B5 = ("block5", "block5", "lds", "block3")  # block5 under auto; DCT_MLP_BLOCK=0 / 3 skip it
B8 = ("block5_b8", "block5_b8", "lds", "lds")  # mlp_block3_ok: batch <= 4, so DCT_MLP_BLOCK=3 falls to the LDS trainer
KERNELS_TRAIN = [([5, 64, 2], 4, WAVE2), (W3, 4, B5), ([5, 64, 2], 3, WAVE2),
                 ([9, 48, 64, 3], 4, ("wave_single", "lds", "lds", "lds")),
                 ([16, 32, 48, 32, 3], 16, ALL_LDS), (W3, 16, ALL_LDS),  # mlp_block5_shape_ok: batch <= 8
                 ([7, 20, 2], 9, ALL_LDS), ([7, 20, 2], 8, WAVE2), ([12, 40, 4], 6, WAVE2), ([16, 64, 3], 2, WAVE2),
                 ([5, 64, 2], 1, WAVE2), ([3, 128, 128, 2], 3, B5), ([8, 128, 128, 2], 1, B5),
                 ([1, 128, 128, 2], 2, B5), (W3, 8, B8), ([8, 128, 128, 2], 5, B8), ([3, 128, 128, 2], 7, B8),
                 (W3, 6, B8)]
# test_fused_grad_mode_matches_autograd's shapes x KERNELS
WAVE_G = ("wave_single", "lds", "lds", "lds")
B3 = ("block3", "block3", "lds", "block3")  # D0 > 8 or classes != 2: mlp_block5_shape_ok refuses, mlp_block3_ok takes
KERNELS_GRAD = [([5, 64, 2], 4, WAVE_G), (W3, 4, B5), ([12, 40, 40, 5], 13, ALL_LDS),  # 5 classes: no wave kernel
                ([9, 48, 64, 3], 4, WAVE_G), ([20, 128, 128, 4], 3, B3), ([32, 128, 128, 1], 4, B3),
                ([8, 128, 128, 2], 3, B5), ([2, 128, 128, 2], 1, B5), (W3, 8, B8), ([7, 128, 128, 2], 6, B8)]
for cases, query in ((KERNELS_TRAIN, TRAIN), (KERNELS_GRAD, GRAD)):
    for dims, B, wants in cases:
        for env, want in zip(KERNEL_ENVS, wants):
            TABLE.append(_row(dims, B, env, query, want))
# ---- edges
TABLE += [
    _row(W3, 4, AUTO, dict(aligned=False), "lds"),  # block5 and block3 both need p on a 16-byte boundary
    _row(W3, 4, AUTO, dict(prof=True), "block5"),  # the one-micro-batch kernels have a profiling instantiation
    _row(W3, 6, AUTO, dict(prof=True), "lds"),  # mlp_block5_ok b8_ok: none at batch 5..8; block3: batch <= 4
    _row(W3, 4, BLOCK8, TRAIN, "block5_b8"),  # DCT_MLP_BLOCK=8: the b8 kernels at every batch
    _row(W3, 2, BLOCK8, TRAIN, "block5_b8"),
    _row(W3, 4, BLOCK8, dict(prof=True), "block3"),  # b8_ok refuses prof; blk == 8 != 0 lets block3 take it
    _row([5, 64, 2], 4, AUTO, TRAIN, "tile", bmax=1024),  # a 1024-plan launches tile at any batch
    _row(W3, 1024, AUTO, TRAIN, "tile"),
    _row(W3, 1025, AUTO, TRAIN, "none", bmax=1024),  # dct_mlp_tile_train: batch <= 1024
    _row(W3, 4, TILE, TRAIN, "tile"),  # DCT_MLP_BLOCK=tile on a tileable shape
    _row([7, 20, 2], 8, TILE, TRAIN, "wave_rows"),  # hidden 20 is not tileable: the knob is reset to auto
    _row([40, 128, 128, 2], 4, TILE, TRAIN, "lds"),  # D0 > 32: not tileable, and neither block kernel's shape
    _row([7, 128, 128, 2], 4, AUTO, TRAIN, "block5"),  # D0 <= 8 (blk5::DMAX)
    _row([9, 128, 128, 2], 4, AUTO, TRAIN, "block3"),  # D0 > 8
    _row([30, 128, 128, 3], 3, AUTO, TRAIN, "block3"),
    _row([5, 64, 2], 4, AUTO, TRAIN, "wave_rows"),  # train against grad mode: rows_eligible's mode == 0
    _row([5, 64, 2], 4, AUTO, GRAD, "wave_single"),
    _row([5, 64, 2], 4, AUTO, dict(stage=True), "wave_single"),  # rows_eligible: no staged batches
    _row([5, 64, 2], 8, AUTO, dict(mode=1, pending=True), "wave_single"),  # update-then-grad
    _row(W3, 4, AUTO, dict(mode=1, pending=True), "none"),  # make_train_args: pending needs a wave plan
    _row([5, 64, 2], 4, AUTO, dict(world=2), "wave_rows"),  # the wave kernels exchange at 2 .. 8 ranks
    _row([5, 64, 2], 4, AUTO, dict(world=8, rank=7), "wave_rows"),
    _row([5, 64, 2], 4, AUTO, dict(world=9), "none"),  # dct_mlp_wave_train: XG_MAXW
    _row([5, 64, 2], 4, AUTO, dict(world=2, rank=2), "none"),  # rank outside the world
    _row([5, 64, 2], 4, LDS, dict(world=2), "none"),  # make_train_args: neither wave nor block5
    _row([9, 48, 64, 3], 4, AUTO, dict(world=2), "none"),  # dct_mlp_wave_train: exchange launches need L == 2
    _row(W3, 5, AUTO, TRAIN, "none", bmax=4),  # dct_mlp_train: batch > bmax
    _row(W3, 4, AUTO, dict(mode=1, world=2), "none"),  # block5 exchanges in train mode only
    _row(W3, 4, BLOCK0, dict(world=2), "block5"),  # dct_mlp_train's exchange branch does not ask DCT_MLP_BLOCK
    _row(W3, 4, AUTO, dict(world=3, prof=True), "none"),  # profiling instantiations at 2 / 4 / 8 ranks only
]
for world in (2, 3, 8):
    TABLE.append(_row(W3, 4, AUTO, dict(world=world), "block5"))  # b5_xg_world_ok: 2 .. 8 ranks
    TABLE.append(_row(W3, 8, AUTO, dict(world=world), "block5_b8"))
TABLE += [_row(W3, 4, AUTO, dict(world=9), "none"), _row(W3, 8, AUTO, dict(world=9), "none")]


@pytest.fixture
def nat(monkeypatch):
    """The selector is host code of the native extension: a build or import failure fails these tests."""
    for k in ("DCT_MLP_KERNEL", "DCT_MLP_BLOCK"):
        monkeypatch.delenv(k, raising=False)
    n = _native.native()
    yield n
    monkeypatch.undo()
    n.reload_knobs()


def _plan(nat, monkeypatch, dims, bmax, env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    return nat.MlpPlan(dims, bmax)  # the constructor re-reads the knobs


def _id(row):
    dims, bmax, env, query, want = row
    q = ",".join("%s=%s" % kv for kv in sorted(query.items()))
    e = ",".join(v for _, v in sorted(env.items())) or "auto"
    return "%s-bmax%d-%s-%s" % ("x".join(map(str, dims)), bmax, e, q)


@pytest.mark.parametrize("row", TABLE, ids=_id)
def test_trainer_of_a_launch(row, nat, monkeypatch):
    dims, bmax, env, query, want = row
    assert _plan(nat, monkeypatch, dims, bmax, env).trainer(**query) == want


def test_stage_is_kept_only_where_a_kernel_reads_it(nat, monkeypatch):
    """dct_mlp_train used to strip MlpArgs::stage and call itself again: now the choice says so."""
    b5 = _plan(nat, monkeypatch, W3, 4, AUTO)
    assert b5.trainer(4, mode=0, stage=True) == "block5" and not b5.uses_stage(4, mode=0, stage=True)
    assert b5.trainer(4, mode=1, stage=True) == "block5" and b5.uses_stage(4, mode=1, stage=True)
    assert not b5.uses_stage(4, mode=1)
    b3 = _plan(nat, monkeypatch, [9, 128, 128, 2], 4, AUTO)
    assert b3.trainer(4, mode=1, stage=True) == "block3" and not b3.uses_stage(4, mode=1, stage=True)
    lds = _plan(nat, monkeypatch, [5, 64, 2], 16, AUTO)
    assert lds.trainer(16, mode=1, stage=True) == "lds" and not lds.uses_stage(16, mode=1, stage=True)
    assert lds.trainer(4, mode=1, stage=True) == "wave_single" and lds.uses_stage(4, mode=1, stage=True)


def test_shape_checks_are_the_native_ones(nat):
    assert nat.mlp_supported(W3, 4) and nat.mlp_supported(W3, 1024) and not nat.mlp_supported(W3, 1025)
    assert not nat.mlp_supported(W3, 0) and not nat.mlp_supported([5, 2], 4)
    assert nat.mlp_supported([5, 64, 2], 16) and not nat.mlp_supported([16, 32, 48, 32, 3], 17)  # 4 layers: no tile
    assert nat.mlp_wave_supported([5, 64, 2], 8) and not nat.mlp_wave_supported([5, 64, 2], 9)
    assert nat.mlp_tile_supported([7, 48, 32, 3]) and not nat.mlp_tile_supported([7, 20, 2])
