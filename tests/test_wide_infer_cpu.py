"""The wide bf16 inference path without a GPU: the predicate's shape set, the evaluation path's choice, the tile
family's pinned answers, and the GPU cases' seeds against the ambiguity cap."""
import pytest
import torch

import infer_cases as ic
import test_wide_infer_gpu as wg

import dct_amd  # noqa: F401
from dct_amd.models.mlp import MLPClassifier
from dct_amd.ops.fused_mlp import FusedMLPKernel
from dct_amd.trainer.evaluate import native_path

CUDA = torch.device("cuda", 0)


def test_predicate_takes_the_wide_shape_set_only():
    ok = FusedMLPKernel.wide_infer_supported
    for c in wg.CASES.values():
        assert ok(c["dims"]) and ok(c["dims"], "gelu")
    for dims in ([8, 1024, 2], [256, 1000, 2], [256, 1024, 9], [32, 128, 128, 128, 128, 2], [256, 1024, 1], [1056, 128, 2]):
        assert not ok(dims)
    assert not ok([32, 128, 2], "silu") and not ok([32, 128, 2], "gelu_tanh")
    assert not ok([256, 1024, 2], norm="layer") and not ok([256, 1024, 1024, 2], residual=True)


@pytest.mark.parametrize("stage", ["val", "test", "predict"])
def test_native_path_takes_the_wide_mlp_on_the_gpu_only(stage):
    model = MLPClassifier(256, hidden=(1024, 1024, 1024), dropout=0.0)
    assert native_path(model, CUDA, stage) and not native_path(model, torch.device("cpu"), stage)
    assert not native_path(MLPClassifier(256, hidden=(1024, 1024), norm="layer"), CUDA, stage)
    assert not native_path(MLPClassifier(256, hidden=(1024, 1024), residual=True), CUDA, stage)
    assert not native_path(MLPClassifier(256, hidden=(1000,)), CUDA, stage)


def test_tile_familys_predicate_keeps_its_answers():
    for dims in ic.SHAPES + [[32, 128, 2]]:  # ([32, 128(, 128), C <= 4] lies in both sets: the evaluation path keeps
        assert FusedMLPKernel.infer_supported(dims)  # it on the fp32 tile kernel)
    for dims in ([64, 256, 128, 3], [256, 1024, 1024, 1024, 2], [96, 384, 8], [33, 64, 2], [5, 24, 2], [5, 64, 5],
                 [5, 64, 64, 64, 2]):
        assert not FusedMLPKernel.infer_supported(dims)


@pytest.mark.parametrize("case", wg.CASES)
def test_seed_keeps_the_ambiguous_rows_under_the_cap(case):
    """With the bound of torch's bf16 forward on the CPU (the GPU test measures it there)."""
    tz, _ = wg.torch_error(case, "cpu")
    gap = wg.reference(case)["gap"]
    for n in wg.ROWS:
        assert int((gap[:n] < 2 * wg.LIMIT * tz).sum()) <= ic.MAX_AMBIGUOUS * n
