"""The skip connection (residual=True) and RMSNorm (norm="rms") options without a GPU: the model class, the packaged
score.py and the trainer selection (csrc/mlp_select.cpp)."""
import importlib.util

import pytest
import torch
import torch.nn.functional as F

from dct_amd.deploy.package import write_score_py
from dct_amd.models.mlp import MLPClassifier, WeatherClassifier, build_mlp
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import mlp_num_params


def test_model_class_takes_and_records_the_options():
    for kw in (dict(norm="batch"), dict(residual=True), dict(hidden=(64, 32), residual=True)):
        with pytest.raises(ValueError):
            MLPClassifier(5, **kw)
    plain = WeatherClassifier(5, residual=False)
    assert plain.hparams == {"input_dim": 5} and "residual" not in plain.fused_spec()
    m = WeatherClassifier(5, norm="rms")
    assert m.hparams == {"input_dim": 5, "norm": "rms"} and m.fused_spec()["norm"] == "rms"
    deep = build_mlp("weather-mlp-3x128", 5, norm="rms", residual=True)
    assert deep.hparams["residual"] is True and deep.fused_spec()["residual"] is True
    assert [k for k in deep.state_dict() if k.startswith("norms")] == ["norms.0.weight", "norms.1.weight"]
    assert sum(t.numel() for t in deep.parameters()) == mlp_num_params(deep.dims, "rms") == mlp_num_params(deep.dims) + 256


@pytest.mark.parametrize("norm", [None, "layer", "rms"])
def test_forward_is_the_formula_and_score_py_rebuilds_it(norm, tmp_path):
    torch.manual_seed(3)
    m = MLPClassifier(5, hidden=(16, 16), activation="gelu", norm=norm, residual=True).double().eval()
    for n in m.norm_layers():
        torch.nn.init.uniform_(n.weight, 0.5, 1.5)
    x = torch.randn(9, 5, dtype=torch.float64)

    def normed(z, i):
        if norm == "rms":
            return m.norms[i].weight * z / torch.sqrt((z * z).mean(-1, keepdim=True) + 1e-5)
        return z if norm is None else F.layer_norm(z, (16,), m.norms[i].weight, m.norms[i].bias, 1e-5)
    h1 = F.gelu(normed(m.net[0](x), 0))
    assert torch.allclose(m(x), m.net[6](h1 + F.gelu(normed(m.net[3](h1), 1))), rtol=1e-12, atol=1e-12)
    write_score_py(str(tmp_path / "score.py"), 5, (16, 16), 0.2, 2, activation="gelu", norm=norm, residual=True)
    spec = importlib.util.spec_from_file_location(f"score_res_{norm}", str(tmp_path / "score.py"))
    score = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(score)
    packed = score.WeatherClassifier(5).double().eval()
    packed.load_state_dict(m.state_dict())
    assert torch.equal(packed(x), m(x))


def test_selection():
    Plan = native().MlpPlan
    for kw in (dict(residual=True), dict(norm="rms"), dict(residual=True, norm="rms")):
        assert Plan([5, 128, 128, 2], 1024).trainer(40, **kw) == Plan([5, 128, 128, 2], 1024).trainer(4, mode=1, **kw) == "tile"
        assert Plan([5, 128, 128, 2], 4).trainer(4, **kw) == Plan([5, 128, 128, 2], 16).trainer(4, **kw) == "none"
    # two hidden layers of equal width only
    assert Plan([5, 64, 2], 1024).trainer(40, residual=True) == Plan([5, 64, 32, 2], 1024).trainer(40, residual=True) == "none"
