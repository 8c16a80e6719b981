"""The TabTransformer inference path without a GPU: which models the evaluation entry points route to the whole-model
kernel (csrc/tt_infer.hip)."""
import pytest
import torch

import dct_amd  # noqa: F401
from dct_amd.models.tabtransformer import TabTransformer
from dct_amd.ops.nn import tt_infer_supported
from dct_amd.trainer.evaluate import native_path

CUDA = torch.device("cuda", 0)


class _OwnStep(TabTransformer):
    def validation_step(self, batch, batch_idx):
        return super().validation_step(batch, batch_idx)


@pytest.mark.parametrize("stage", ["val", "test", "predict"])
def test_native_path_takes_the_benchmark_shape_on_the_gpu_only(stage):
    model = TabTransformer(num_features=64, d_model=64, heads=4, ffn_mult=4, layers=2, num_classes=3)
    assert native_path(model, CUDA, stage) and not native_path(model, torch.device("cpu"), stage)
    assert not native_path(TabTransformer(d_model=32), CUDA, stage)
    assert not native_path(TabTransformer(num_features=16), CUDA, stage)
    assert native_path(_OwnStep(), CUDA, stage) == (stage != "val")


def test_predicate_takes_one_to_eight_blocks_and_two_to_eight_classes():
    assert tt_infer_supported({}) and tt_infer_supported(dict(layers=1, num_classes=8)) and tt_infer_supported(dict(layers=8))
    for hp in (dict(layers=0), dict(layers=9), dict(num_classes=1), dict(num_classes=9), dict(heads=8), dict(ffn_mult=2)):
        assert not tt_infer_supported(hp)
