"""Trainer(gradient_clip_val, gradient_clip_algorithm) on the CPU: the clipped trajectory against a plain torch loop
(clip_grad_norm_ / clip_grad_value_ before torch.optim.Adam.step()), the argument checks, and the engine routing.

Tolerance of the torch-parity checks: max |dp| < 1e-4, the bound this suite's other comparisons of a trained parameter
vector with a torch.optim.Adam loop use (tests/test_ddp_cpu.py's single-process emulation).  The inputs are scaled so
that the clipped and the unclipped torch trajectories differ by more than 100 times that after the 20 steps: parity
with the clipped loop then says something about clipping."""
import types

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

import dct_amd  # noqa: F401
from dct_amd.data.dataset import TensorPairDataset
from dct_amd.models.mlp import MLPClassifier
from dct_amd.ops.optim import FlatAdam, clip_workspace, grad_clip_coef_
from dct_amd.trainer import Trainer
from dct_amd.trainer import trainer as trainer_mod

TOL = 1e-4
STEPS, B, D = 20, 16, 8
CLIP_NORM = 0.05
CLIP_VALUE = 0.01
X_SCALE = 4.0  # features ~ N(0, 4^2): gradient norms between ~0.3 and ~5 over the 20 steps, all above CLIP_NORM


def _data():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(STEPS * B, D, generator=gen) * X_SCALE
    y = (x[:, 0] + 0.5 * x[:, 1] * x[:, 2] / X_SCALE > 0).long()
    return x, y


def _model():
    torch.manual_seed(3)
    return MLPClassifier(D, hidden=(32,), dropout=0.0)


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()


def _torch_loop(clip_val, algorithm):
    x, y = _data()
    model = _model()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    params = list(model.parameters())
    norms = []
    for s in range(STEPS):
        opt.zero_grad()
        F.cross_entropy(model(x[s * B:(s + 1) * B]), y[s * B:(s + 1) * B]).backward()
        if clip_val is not None:
            if algorithm == "norm":
                norms.append(float(torch.nn.utils.clip_grad_norm_(params, clip_val)))
            else:
                torch.nn.utils.clip_grad_value_(params, clip_val)
        opt.step()
    return _flat(model), norms


def _trainer_run(**clip):
    x, y = _data()
    model = _model()
    t = Trainer(max_epochs=1, accelerator="cpu", engine="autograd", logger=None, num_sanity_val_steps=0, verbose=False,
                enable_progress_bar=False, **clip)
    t.fit(model, DataLoader(TensorPairDataset(x, y), batch_size=B, shuffle=False),
          DataLoader(TensorPairDataset(x[:B], y[:B]), batch_size=B))
    assert t.global_step == STEPS
    return _flat(model), t


def test_unclipped_trainer_matches_torch():
    got, _ = _trainer_run()
    want, _ = _torch_loop(None, "norm")
    assert (got - want).abs().max() < TOL


@pytest.mark.parametrize("algorithm,val", [("norm", CLIP_NORM), ("value", CLIP_VALUE)])
def test_clipped_trainer_matches_clipped_torch_loop(algorithm, val):
    want, norms = _torch_loop(val, algorithm)
    unclipped, _ = _torch_loop(None, algorithm)
    gap = float((want - unclipped).abs().max())
    print("clipped vs unclipped torch trajectories after %d steps: max |dp| = %.4f" % (STEPS, gap))
    assert gap > 100 * TOL, "the inputs do not make clipping matter"
    if norms:
        assert min(norms) > val  # every step clips
    got, t = _trainer_run(gradient_clip_val=val, gradient_clip_algorithm=algorithm)
    err = float((got - want).abs().max())
    print("Trainer(%s=%g) vs the clipped torch loop: max |dp| = %.3e" % (algorithm, val, err))
    assert err < TOL
    norm, coef = t.engine.grad_clip_stats()
    if algorithm == "norm":
        assert norm == pytest.approx(norms[-1], rel=1e-5) and coef == pytest.approx(val / (norms[-1] + 1e-6), rel=1e-5)
    else:
        assert norm != norm and coef == 1.0


class _SgdClassifier(MLPClassifier):
    def configure_optimizers(self):
        return torch.optim.SGD(self.parameters(), lr=0.05, momentum=0.9)


@pytest.mark.parametrize("algorithm,val", [("norm", CLIP_NORM), ("value", CLIP_VALUE)])
def test_non_adam_optimizer_clips_with_the_torch_functions(algorithm, val):
    """A module whose optimizer is not Adam keeps its torch optimizer; the engine then calls clip_grad_norm_ /
    clip_grad_value_ on the parameters before its step (and p.grad IS rewritten, as in torch)."""
    x, y = _data()

    def loop(clip):
        torch.manual_seed(3)
        model = _SgdClassifier(D, hidden=(32,), dropout=0.0)
        opt = model.configure_optimizers()
        params, norms = list(model.parameters()), []
        for s in range(STEPS):
            opt.zero_grad()
            F.cross_entropy(model(x[s * B:(s + 1) * B]), y[s * B:(s + 1) * B]).backward()
            if clip and algorithm == "norm":
                norms.append(float(torch.nn.utils.clip_grad_norm_(params, val)))
            elif clip:
                torch.nn.utils.clip_grad_value_(params, val)
            opt.step()
        return _flat(model), norms

    want, norms = loop(True)
    assert float((want - loop(False)[0]).abs().max()) > 100 * TOL, "the inputs do not make clipping matter"
    torch.manual_seed(3)
    model = _SgdClassifier(D, hidden=(32,), dropout=0.0)
    t = Trainer(max_epochs=1, accelerator="cpu", engine="autograd", logger=None, num_sanity_val_steps=0, verbose=False,
                enable_progress_bar=False, gradient_clip_val=val, gradient_clip_algorithm=algorithm)
    t.fit(model, DataLoader(TensorPairDataset(x, y), batch_size=B, shuffle=False),
          DataLoader(TensorPairDataset(x[:B], y[:B]), batch_size=B))
    assert t.engine.optimizer is None and isinstance(t.engine.torch_optimizer, torch.optim.SGD)
    assert float((_flat(model) - want).abs().max()) < TOL
    norm, coef = t.engine.grad_clip_stats()
    if algorithm == "norm":
        assert norm == pytest.approx(norms[-1], rel=1e-5) and coef == pytest.approx(val / (norms[-1] + 1e-6), rel=1e-5)
        g = torch.cat([p.grad.reshape(-1) for p in t.engine.params])
        assert float(g.norm()) == pytest.approx(val, rel=1e-4)  # rewritten in place
    else:
        assert norm != norm and coef == 1.0


def test_gradient_stays_unclipped_in_p_grad():
    """The documented difference from torch: the clip is applied inside Adam, p.grad keeps the unclipped gradient."""
    _, t = _trainer_run(gradient_clip_val=CLIP_NORM)
    norm, coef = t.engine.grad_clip_stats()
    g = torch.cat([p.grad.reshape(-1) for p in t.engine.params])
    assert float(g.norm()) == pytest.approx(norm, rel=1e-6) and norm > CLIP_NORM and coef < 1.0


@pytest.mark.parametrize("val", [None, 0, 0.0])
def test_none_and_zero_mean_off(val):
    t = Trainer(accelerator="cpu", gradient_clip_val=val, verbose=False)
    assert t.gradient_clip_val is None and t.gradient_clip_algorithm == "norm"


@pytest.mark.parametrize("kw", [dict(gradient_clip_val=-1.0), dict(gradient_clip_val=float("nan")),
                                dict(gradient_clip_val=1.0, gradient_clip_algorithm="l1"),
                                dict(gradient_clip_algorithm="nrom")])
def test_bad_arguments_raise_value_error(kw):
    with pytest.raises(ValueError):
        Trainer(accelerator="cpu", verbose=False, **kw)


class _Fake:
    ok = True

    def __init__(self, *a, **kw):
        self.kw = kw

    @classmethod
    def applicable(cls, *a, **kw):
        return cls.ok


def _routed(monkeypatch, engine, batch, fused_ok=True, graph_ok=True, **clip):
    """The class _make_engine picks, with every engine replaced by a recording stand-in (no device needed)."""
    fakes = {n: type(n, (_Fake,), {}) for n in ("FusedMLPEngine", "GraphMLPEngine", "AutogradEngine")}
    fakes["FusedMLPEngine"].ok, fakes["GraphMLPEngine"].ok = fused_ok, graph_ok
    for n, c in fakes.items():
        monkeypatch.setattr(trainer_mod, n, c)
    monkeypatch.delenv("DCT_ENGINE", raising=False)
    t = Trainer(accelerator="cpu", engine=engine, verbose=False, **clip)
    t.ctx = types.SimpleNamespace(device=torch.device("cpu"))
    e = t._make_engine(_model(), batch, 0)
    return type(e).__name__, e.kw


def test_engine_routing_is_unchanged_without_clipping(monkeypatch):
    assert _routed(monkeypatch, "auto", 4)[0] == "FusedMLPEngine"
    assert _routed(monkeypatch, "auto", 64)[0] == "GraphMLPEngine"       # batch > 16: the graph engine keeps its models
    assert _routed(monkeypatch, "auto", 64, graph_ok=False)[0] == "FusedMLPEngine"
    assert _routed(monkeypatch, "fused", 4)[0] == "FusedMLPEngine"
    assert _routed(monkeypatch, "auto", 4, gradient_clip_val=0)[0] == "FusedMLPEngine"
    name, kw = _routed(monkeypatch, "auto", 4, fused_ok=False, graph_ok=False)
    assert name == "AutogradEngine" and kw["gradient_clip_val"] is None


def test_clipping_routes_around_the_fused_engine(monkeypatch):
    name, kw = _routed(monkeypatch, "auto", 4, gradient_clip_val=0.5)
    assert name == "GraphMLPEngine" and kw == dict(gradient_clip_val=0.5, gradient_clip_algorithm="norm")
    name, kw = _routed(monkeypatch, "auto", 4, graph_ok=False, gradient_clip_val=0.5, gradient_clip_algorithm="value")
    assert name == "AutogradEngine" and kw == dict(gradient_clip_val=0.5, gradient_clip_algorithm="value")
    with pytest.raises(RuntimeError, match="cannot clip"):
        _routed(monkeypatch, "fused", 4, gradient_clip_val=0.5)


def test_flat_adam_cpu_clips_with_the_same_formulas():
    gen = torch.Generator().manual_seed(0)
    p0, g = torch.randn(37, generator=gen), torch.randn(37, generator=gen)
    for algorithm, val in (("norm", 0.5), ("value", 0.3)):
        p, q = p0.clone(), p0.clone().requires_grad_()
        FlatAdam(p, g, [p.shape], lr=0.01, clip_val=val, clip_algorithm=algorithm).step()
        q.grad = g.clone()
        (torch.nn.utils.clip_grad_norm_ if algorithm == "norm" else torch.nn.utils.clip_grad_value_)([q], val)
        torch.optim.Adam([q], lr=0.01).step()
        assert (p - q.detach()).abs().max() < 1e-6
    ws = clip_workspace("cpu")
    norm, coef = grad_clip_coef_(g, 1e30, ws).tolist()
    assert norm == pytest.approx(float(g.norm())) and coef == 1.0
    assert float(grad_clip_coef_(g, 0.5, ws, grad_scale=0.5)[0]) == pytest.approx(0.5 * float(g.norm()))


def test_config_and_job_flags():
    import importlib.util
    import os

    from dct_amd.config import default_config

    cfg = default_config({})
    assert cfg.optim.gradient_clip_val is None and cfg.optim.gradient_clip_algorithm == "norm"
    from dct_amd.config import PipelineConfig

    cfg = PipelineConfig.from_dict({"optim": {"gradient_clip_val": 0.5, "gradient_clip_algorithm": "value"}})
    assert cfg.optim.gradient_clip_val == 0.5 and cfg.optim.gradient_clip_algorithm == "value"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_ddp_job", os.path.join(root, "jobs", "train_ddp.py"))
    job = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(job)
    a = job.parse_args([])
    assert a.gradient_clip_val is None and a.gradient_clip_algorithm == "norm"
    a = job.parse_args(["--gradient-clip-val", "0.5", "--gradient-clip-algorithm", "value"])
    assert a.gradient_clip_val == 0.5 and a.gradient_clip_algorithm == "value"
