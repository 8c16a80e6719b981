"""The hidden-layer LayerNorm option (norm=None / "layer") without a GPU: the model class, the trainer selection
(csrc/mlp_select.cpp) and the packaged score.py."""
import importlib.util

import pytest
import torch

from dct_amd.ckpt.lightning_io import build_checkpoint, save_checkpoint
from dct_amd.deploy.package import write_score_py
from dct_amd.models.mlp import MLPClassifier, WeatherClassifier, build_mlp
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import mlp_num_params


def test_model_class_records_the_norm_only_when_set():
    with pytest.raises(ValueError):
        MLPClassifier(5, norm="batch")
    plain = WeatherClassifier(5)
    assert plain.hparams == {"input_dim": 5} and WeatherClassifier(5, norm=None).hparams == {"input_dim": 5}
    assert list(plain.state_dict()) == ["net.0.weight", "net.0.bias", "net.3.weight", "net.3.bias"]
    assert plain.fused_spec() == {"dims": [5, 64, 2], "dropout": 0.2, "loss": "ce"}
    m = WeatherClassifier(5, norm="layer")
    assert m.hparams == {"input_dim": 5, "norm": "layer"} and m.fused_spec()["norm"] == "layer"
    assert list(m.state_dict()) == list(plain.state_dict()) + ["norms.0.weight", "norms.0.bias"]
    deep = build_mlp("weather-mlp-3x128", 5, norm="layer", activation="gelu")
    assert [k for k in deep.state_dict() if k.startswith("norms")] == [
        "norms.0.weight", "norms.0.bias", "norms.1.weight", "norms.1.bias"]
    # parameters() order is the kernels' flat order: all linears, then gamma_1, beta_1, gamma_2, beta_2
    assert [tuple(t.shape) for t in deep.parameters()][-4:] == [(128,)] * 4
    assert sum(t.numel() for t in deep.parameters()) == mlp_num_params(deep.dims, "layer")


def test_selection():
    Plan = native().MlpPlan
    tile = Plan([5, 128, 128, 2], 1024)
    assert [tile.trainer(B, norm="layer") for B in (4, 40, 1024, 1025)] == ["tile", "tile", "tile", "none"]
    assert tile.trainer(4, mode=1, norm="layer") == "tile"  # grad mode honours it: part of the model
    assert tile.trainer(4, world=2, norm="layer") == "none"
    for plan in (Plan([5, 128, 128, 2], 4), Plan([5, 128, 128, 2], 16), Plan([5, 64, 2], 4), Plan([5, 300, 2], 1024)):
        assert plan.trainer(4, norm="layer") == "none" and plan.trainer(4, mode=1, norm="layer") == "none"
    # the slots follow the longer P (642 words, stride 644); without a norm the workspace is what it was
    assert native().mlp_tile_ws_floats_norm([5, 64, 2], 40, 1, "layer") == 2 * 644 + 4
    assert native().mlp_tile_ws_floats_norm([5, 64, 2], 40, 3) == native().mlp_tile_ws_floats_accum([5, 64, 2], 40, 3)


@pytest.mark.parametrize("norm", ["layer", None])
def test_packaged_score_py_rebuilds_the_saved_model(tmp_path, norm):
    torch.manual_seed(5)
    model = MLPClassifier(5, hidden=(16, 32), dropout=0.0, **({} if norm is None else {"norm": norm})).eval()
    if norm is not None:
        with torch.no_grad():
            for ln in model.norm_layers():
                ln.weight.uniform_(0.5, 1.5)
                ln.bias.uniform_(-0.5, 0.5)
    hp = dict(model.hparams)
    assert ("norm" in hp) == (norm is not None)
    save_checkpoint(build_checkpoint(model.state_dict(), epoch=0, global_step=1, hyper_parameters=hp),
                    str(tmp_path / "model.ckpt"))
    write_score_py(str(tmp_path / "score.py"), 5, hp["hidden"], 0.0, 2, norm=hp.get("norm"))
    spec = importlib.util.spec_from_file_location(f"score_norm_{norm}", str(tmp_path / "score.py"))
    score = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(score)
    score.init()
    x = torch.randn(9, 5)
    with torch.no_grad():
        assert torch.equal(score._model(x), model(x))
        assert list(score._model.state_dict()) == list(model.state_dict())
