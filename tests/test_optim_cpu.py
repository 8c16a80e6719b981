"""AdamW and SGD on the fused engine, without a GPU: which optimizers the engine takes (optim_hparams_of), the Trainer's
routing (recording stand-ins), the plan's answer for a non-Adam launch, the argument checks, the config and the
command-line flags down to the model's torch optimizer, FlatSGD's CPU path against torch.optim.SGD, and the layout of
MlpArgs (the new fields last)."""
import glob
import importlib.util
import os
import re
import types

import pytest
import torch

import dct_amd  # noqa: F401
import dct_amd.trainer.trainer as trainer_mod
from dct_amd.config import OptimConfig, optimizer_kwargs
from dct_amd.models import build_model
from dct_amd.models.mlp import MLPClassifier, WeatherClassifier
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import FusedMLPKernel, check_optimizer
from dct_amd.ops.optim import FlatSGD
from dct_amd.trainer import Trainer
from dct_amd.trainer.engines import FusedMLPEngine, adam_hparams_from, adam_hparams_of, optim_hparams_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params():
    return [torch.zeros(3, requires_grad=True)]


# ------------------------------------------------------------------------------------------------ hyper-parameters
def test_optim_hparams_of():
    adam = torch.optim.Adam(_params(), lr=0.02, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1)
    want = dict(lr=0.02, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1)
    assert optim_hparams_of(adam) == adam_hparams_of(adam) == want  # no new key for Adam
    adamw = torch.optim.AdamW(_params(), lr=0.02, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1)
    assert optim_hparams_of(adamw) == dict(want, kind="adamw") and adam_hparams_of(adamw) is None
    sgd = torch.optim.SGD(_params(), lr=0.1, momentum=0.9, dampening=0.0, nesterov=True, weight_decay=0.05)
    assert optim_hparams_of(sgd) == dict(kind="sgd", lr=0.1, momentum=0.9, dampening=0.0, nesterov=True,
                                         weight_decay=0.05)
    assert adam_hparams_of(sgd) is None and adam_hparams_from(sgd) is None
    assert optim_hparams_of(torch.optim.SGD(_params(), lr=0.1))["momentum"] == 0.0
    # everything else keeps the torch optimizer
    assert optim_hparams_of(torch.optim.AdamW(_params(), amsgrad=True)) is None
    assert optim_hparams_of(torch.optim.Adam(_params(), amsgrad=True)) is None
    assert optim_hparams_of(torch.optim.SGD(_params(), lr=0.1, maximize=True)) is None
    assert optim_hparams_of(torch.optim.AdamW(_params(), maximize=True)) is None
    assert optim_hparams_of(torch.optim.RMSprop(_params())) is None
    a, b = torch.zeros(2, requires_grad=True), torch.zeros(2, requires_grad=True)
    groups = [dict(params=[a]), dict(params=[b], momentum=0.5)]
    assert optim_hparams_of(torch.optim.SGD(groups, lr=0.1, momentum=0.9)) is None
    same = [dict(params=[a]), dict(params=[b])]
    assert optim_hparams_of(torch.optim.SGD(same, lr=0.1, momentum=0.9))["momentum"] == 0.9


# ------------------------------------------------------------------------------------------------ routing
class _Fake:
    ok = True

    def __init__(self, *a, **kw):
        self.a, self.kw = a, kw

    @classmethod
    def applicable(cls, *a, **kw):
        cls.asked, cls.asked_kw = a[3:], kw
        return cls.ok


def _routed(monkeypatch, engine, batch, model, fused_ok=True, graph_ok=True, **kw):
    fakes = {n: type(n, (_Fake,), {}) for n in ("FusedMLPEngine", "GraphMLPEngine", "AutogradEngine")}
    fakes["FusedMLPEngine"].ok, fakes["GraphMLPEngine"].ok = fused_ok, graph_ok
    for n, c in fakes.items():
        monkeypatch.setattr(trainer_mod, n, c)
    monkeypatch.delenv("DCT_ENGINE", raising=False)
    t = Trainer(accelerator="cpu", engine=engine, verbose=False, **kw)
    t.ctx = types.SimpleNamespace(device=torch.device("cpu"))
    e = t._make_engine(model, batch, 0)
    return type(e).__name__, e, fakes


def _sgd():
    return MLPClassifier(5, hidden=(64,), dropout=0.0, optimizer="sgd", momentum=0.9, nesterov=True)


def test_a_non_adam_model_takes_the_fused_engine_where_it_applies(monkeypatch):
    for batch in (4, 64):  # also above 16, where the graph engine would take an Adam model
        name, e, fakes = _routed(monkeypatch, "auto", batch, _sgd())
        assert name == "FusedMLPEngine"
        assert fakes["FusedMLPEngine"].asked == () and fakes["FusedMLPEngine"].asked_kw == dict(optimizer="sgd")
        assert e.a[4] == dict(kind="sgd", lr=0.01, momentum=0.9, dampening=0.0, nesterov=True, weight_decay=0.0)
    name, e, fakes = _routed(monkeypatch, "auto", 64, MLPClassifier(5, dropout=0.0, optimizer="adamw", weight_decay=0.05))
    assert name == "FusedMLPEngine" and fakes["FusedMLPEngine"].asked_kw == dict(optimizer="adamw")
    assert e.a[4]["kind"] == "adamw" and e.a[4]["weight_decay"] == 0.05
    # with accumulation the window argument comes first, as before
    name, e, fakes = _routed(monkeypatch, "auto", 4, _sgd(), accumulate_grad_batches=3)
    assert name == "FusedMLPEngine" and fakes["FusedMLPEngine"].asked == (3,)
    assert fakes["FusedMLPEngine"].asked_kw == dict(optimizer="sgd")
    # not applicable: autograd with the torch optimizer, never the graph engine
    for batch in (4, 64):
        assert _routed(monkeypatch, "auto", batch, _sgd(), fused_ok=False)[0] == "AutogradEngine"
    with pytest.raises(RuntimeError, match="not supported"):
        _routed(monkeypatch, "fused", 4, _sgd(), fused_ok=False)
    with pytest.raises(RuntimeError, match="not supported"):  # engine="graph": as before, it knows only Adam
        _routed(monkeypatch, "graph", 64, _sgd())
    # clipping still routes around the fused engine
    assert _routed(monkeypatch, "auto", 4, _sgd(), gradient_clip_val=0.5)[0] == "AutogradEngine"


def test_adam_routing_asks_applicable_as_before(monkeypatch):
    adam = MLPClassifier(5, hidden=(64,), dropout=0.0)
    name, e, fakes = _routed(monkeypatch, "auto", 4, adam)
    assert name == "FusedMLPEngine" and fakes["FusedMLPEngine"].asked == () and fakes["FusedMLPEngine"].asked_kw == {}
    assert e.a[4] == dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    assert _routed(monkeypatch, "auto", 64, adam)[0] == "GraphMLPEngine"


def test_an_optimizer_the_engine_does_not_know_goes_to_autograd(monkeypatch):
    class Rms(MLPClassifier):
        def configure_optimizers(self):
            return torch.optim.RMSprop(self.parameters(), lr=0.01)

    assert _routed(monkeypatch, "auto", 4, Rms(5, dropout=0.0))[0] == "AutogradEngine"
    ams = MLPClassifier(5, dropout=0.0)
    ams.configure_optimizers = lambda: torch.optim.AdamW(ams.parameters(), amsgrad=True)
    assert _routed(monkeypatch, "auto", 4, ams)[0] == "AutogradEngine"


def test_fused_engine_applicable_follows_the_tile_plan():
    dev = torch.device("cuda")  # (applicable only looks at the type)
    small, wide = MLPClassifier(5, hidden=(64,), dropout=0.0), MLPClassifier(5, hidden=(256,), dropout=0.0)
    for kind in ("sgd", "adamw"):
        for B in (1, 4, 16, 17, 1024):
            assert FusedMLPEngine.applicable(small, dev, B, optimizer=kind)
        assert not FusedMLPEngine.applicable(small, dev, 1025, optimizer=kind)
        assert not FusedMLPEngine.applicable(wide, dev, 4, optimizer=kind)  # not a tile shape
        assert not FusedMLPEngine.applicable(small, torch.device("cpu"), 4, optimizer=kind)
        assert FusedMLPEngine.applicable(small, dev, 40, 3, optimizer=kind)
    assert FusedMLPEngine.applicable(wide, dev, 4) == FusedMLPEngine.applicable(wide, dev, 4, optimizer="adam")


# ------------------------------------------------------------------------------------------------ the plan, the checks
def test_plan_names_the_trainer_of_a_non_adam_launch():
    nat = native()
    tile = nat.MlpPlan([5, 64, 2], 1024)
    for kind in ("sgd", "adamw"):
        for B in (1, 4, 16, 17, 1024):
            assert tile.trainer(B, optimizer=kind) == "tile"
        assert tile.trainer(1025, optimizer=kind) == "none"
        assert tile.trainer(40, optimizer=kind, world=2) == "none"  # no in-kernel exchange
        assert tile.trainer(40, optimizer=kind, accumulate=3, weighted=True) == "tile"
        for dims, bmax, B in (([5, 64, 2], 4, 4), ([5, 64, 2], 16, 16), ([5, 128, 128, 2], 4, 4), ([12, 40, 4], 16, 6)):
            plan = nat.MlpPlan(dims, bmax)
            assert plan.trainer(B) == plan.trainer(B, optimizer="adam") != "none"
            assert plan.trainer(B, optimizer=kind) == "none"
            assert plan.trainer(B, mode=1, optimizer=kind) == plan.trainer(B, mode=1)  # grad mode applies no optimizer
    assert nat.MlpPlan([5, 300, 2], 16).trainer(4, optimizer="sgd") == "none"  # a non-tile shape
    with pytest.raises(ValueError, match="optimizer"):
        tile.trainer(4, optimizer="rmsprop")


def test_argument_checks():
    assert check_optimizer("adam") == "adam" and check_optimizer("sgd", momentum=0.9, nesterov=True) == "sgd"
    for bad in (dict(optimizer="rmsprop"), dict(optimizer="sgd", momentum=-0.1), dict(optimizer="sgd", weight_decay=-1.0),
                dict(optimizer="adamw", weight_decay=-0.5), dict(optimizer="sgd", nesterov=True),
                dict(optimizer="sgd", nesterov=True, momentum=0.9, dampening=0.1), dict(optimizer=None)):
        with pytest.raises(ValueError):
            check_optimizer(**bad)
        if bad["optimizer"] is not None:
            with pytest.raises(ValueError):
                MLPClassifier(5, **bad)
    # a non-Adam optimizer on a plan that is not the tile trainer's: refused before any operand is looked at
    for bmax, B in ((4, 4), (16, 16)):
        k = FusedMLPKernel([5, 64, 2], bmax=bmax)
        for kind in ("sgd", "adamw"):
            with pytest.raises(ValueError, match="batch-tiled"):
                k.train(None, None, None, None, None, None, n_items=B, batch=B, steps=1, t0=0, lr=0.01, optimizer=kind)
            with pytest.raises(ValueError, match="batch-tiled"):
                k.prepare_train(None, None, None, None, None, None, n_items=B, batch=B, lr=0.01, optimizer=kind)


# ------------------------------------------------------------------------------------------------ model, config, CLI
def test_model_builds_the_matching_torch_optimizer():
    m = MLPClassifier(5)
    o = m.configure_optimizers()
    assert type(o) is torch.optim.Adam and adam_hparams_of(o) == dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8,
                                                                      weight_decay=0.0)
    assert "optimizer" not in m.hparams and "momentum" not in m.hparams and "betas" not in m.hparams
    assert dict(WeatherClassifier(5).hparams) == {"input_dim": 5}
    s = MLPClassifier(5, optimizer="sgd", momentum=0.9, nesterov=True, weight_decay=0.05, lr=0.1)
    assert optim_hparams_of(s.configure_optimizers()) == dict(kind="sgd", lr=0.1, momentum=0.9, dampening=0.0,
                                                              nesterov=True, weight_decay=0.05)
    assert s.hparams["optimizer"] == "sgd" and s.hparams["momentum"] == 0.9 and s.hparams["nesterov"] is True
    w = MLPClassifier(5, optimizer="adamw", weight_decay=0.05, betas=(0.8, 0.99), eps=1e-6)
    assert optim_hparams_of(w.configure_optimizers()) == dict(kind="adamw", lr=0.01, betas=(0.8, 0.99), eps=1e-6,
                                                              weight_decay=0.05)
    again = MLPClassifier(**dict(w.hparams))  # the recorded hyper-parameters rebuild the model
    assert optim_hparams_of(again.configure_optimizers()) == optim_hparams_of(w.configure_optimizers())
    ww = WeatherClassifier(5, optimizer="adamw", weight_decay=0.05)
    assert dict(ww.hparams) == {"input_dim": 5, "optimizer": "adamw", "weight_decay": 0.05}
    assert type(WeatherClassifier(**dict(ww.hparams)).configure_optimizers()) is torch.optim.AdamW


def test_config_reaches_the_model():
    assert optimizer_kwargs(OptimConfig()) == {}
    cfg = OptimConfig(name="sgd", momentum=0.9, nesterov=True, weight_decay=0.01)
    kw = optimizer_kwargs(cfg)
    assert kw == dict(optimizer="sgd", momentum=0.9, nesterov=True, weight_decay=0.01)
    o = build_model("weather", 5, **kw).configure_optimizers()
    assert optim_hparams_of(o) == dict(kind="sgd", lr=0.01, momentum=0.9, dampening=0.0, nesterov=True,
                                       weight_decay=0.01)
    cfg = OptimConfig(name="adamw", betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05)
    o = build_model("weather-mlp-3x128", 5, **optimizer_kwargs(cfg)).configure_optimizers()
    assert optim_hparams_of(o) == dict(kind="adamw", lr=0.01, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05)
    assert OptimConfig(name="sgd", dampening=0.1).dampening == 0.1


def test_command_line_flags_reach_the_model():
    spec = importlib.util.spec_from_file_location("train_ddp_job", os.path.join(ROOT, "jobs", "train_ddp.py"))
    job = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(job)
    a = job.parse_args([])
    assert (a.optimizer, a.weight_decay, a.momentum, a.nesterov) == ("adam", 0.0, 0.0, False)
    assert job.model_optim_kwargs(a) == {}
    a = job.parse_args(["--optimizer", "sgd", "--momentum", "0.9", "--nesterov", "--weight-decay", "0.01"])
    kw = job.model_optim_kwargs(a)
    assert kw == dict(optimizer="sgd", momentum=0.9, nesterov=True, weight_decay=0.01)
    o = build_model(a.model, 5, lr=a.lr, **kw).configure_optimizers()
    assert type(o) is torch.optim.SGD and o.defaults["nesterov"] and o.defaults["momentum"] == 0.9
    a = job.parse_args(["--optimizer", "adamw", "--weight-decay", "0.05"])
    assert type(build_model(a.model, 5, **job.model_optim_kwargs(a)).configure_optimizers()) is torch.optim.AdamW
    with pytest.raises(SystemExit):
        job.parse_args(["--optimizer", "rmsprop"])


# ------------------------------------------------------------------------------------------------ FlatSGD
@pytest.mark.parametrize("hp", [dict(), dict(momentum=0.9), dict(momentum=0.9, dampening=0.1, weight_decay=0.05),
                                dict(momentum=0.9, nesterov=True, weight_decay=0.05)])
def test_flat_sgd_cpu_path_is_torch_sgd_step_by_step(hp):
    g0 = torch.Generator().manual_seed(3)
    shapes = [torch.Size([4, 3]), torch.Size([4])]
    flat = torch.randn(16, generator=g0)
    grad = torch.zeros(16)
    fs = FlatSGD(flat, grad, shapes, lr=0.05, **hp)
    fs.m.fill_(float("nan"))  # the first step ignores what the buffer held
    ref = [flat[:12].clone().view(4, 3).requires_grad_(), flat[12:].clone().requires_grad_()]
    opt = torch.optim.SGD(ref, lr=0.05, **hp)
    assert fs.state_dict()["state"] == {}
    assert set(fs.state_dict()["param_groups"][0]) == set(opt.state_dict()["param_groups"][0])
    for _ in range(4):
        grad.copy_(torch.randn(16, generator=g0))
        ref[0].grad, ref[1].grad = grad[:12].clone().view(4, 3), grad[12:].clone()
        opt.step()
        fs.step()
        want = torch.cat([r.detach().reshape(-1) for r in ref])
        assert torch.allclose(flat, want, rtol=1e-6, atol=1e-7)
    sd, tsd = fs.state_dict(), opt.state_dict()
    assert set(sd["state"]) == set(tsd["state"])  # momentum_buffer per parameter - or no state without momentum
    for i in sd["state"]:
        assert set(sd["state"][i]) == {"momentum_buffer"}
        assert torch.allclose(sd["state"][i]["momentum_buffer"], tsd["state"][i]["momentum_buffer"], rtol=1e-6, atol=1e-7)
        assert sd["state"][i]["momentum_buffer"].shape == shapes[i]
    fresh = torch.optim.SGD([torch.zeros(4, 3, requires_grad=True), torch.zeros(4, requires_grad=True)], lr=1.0)
    fresh.load_state_dict(sd)  # torch takes the layout
    assert fresh.param_groups[0]["lr"] == 0.05 and fresh.param_groups[0]["momentum"] == hp.get("momentum", 0.0)
    other = FlatSGD(flat.clone(), grad, shapes, lr=1.0)
    other.load_state_dict(tsd)
    assert other.param_groups[0]["momentum"] == hp.get("momentum", 0.0) and other.lr == 0.05
    if hp.get("momentum"):
        assert torch.allclose(other.m, fs.m, rtol=1e-6, atol=1e-7) and other.step_count == 1


# ------------------------------------------------------------------------------------------------ MlpArgs
def test_new_mlp_args_fields_sit_after_the_existing_ones():
    """Text only, like tests/test_native_api_cpu.py: the members of struct MlpArgs in declaration order.  Every field
    that was there keeps its place (and so its kernel-argument offset); the optimizer's are appended."""
    (path,) = glob.glob(os.path.join(ROOT, "*", "csrc", "mlp_fused.h"))
    with open(path) as f:
        text = f.read()
    def members(pattern):
        body = re.sub(r"//[^\n]*", "", re.search(pattern, text, re.S).group(1))
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *rest = decl.split(",")
                names += [re.findall(r"\w+", first)[-1]] + [re.findall(r"\w+", r)[-1] for r in rest]
        return names

    # MlpArgs is its prefix MlpStepArgs (the struct as it was: the tile kernels' Adam argument) and the appended fields
    names = members(r"struct MlpStepArgs \{(.*?)\n\};") + members(r"struct MlpArgs : MlpStepArgs \{(.*?)\n\};")
    before = ["p", "m", "v", "grad_out", "X", "ldx", "Y", "idx", "n_items", "B", "steps", "t0", "lr", "b1", "b2", "eps",
              "wd", "dropout", "seed", "step_base", "loss_out", "mode", "loss_kind", "eval_acc", "logits_out",
              "step_counter", "cursor", "prof", "pending", "stage", "xg_recv", "xg_peers", "xg_world", "xg_rank",
              "xg_status", "xg_timeout", "xg_poll", "xg_ticks", "tune", "k_drop_scale", "k_l2b1", "k_l2b2", "k_rc1",
              "k_rc2", "k_sqc2", "tile_ws", "tile_ws_floats", "lr_tab", "class_w", "label_smooth", "accum"]
    assert names[:len(before)] == before
    assert names[len(before):] == ["opt_kind", "momentum", "dampening", "nesterov"]
