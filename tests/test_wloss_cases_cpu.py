"""Class-weighted, label-smoothed cross-entropy on the CPU: the fp64 reference of tests/wloss_cases.py against torch
and against the wrong implementations the GPU tolerances must reject, and every layer above the kernels that needs no
GPU - the model, its hyper-parameters, the plan's trainer query, the engine routing, the job flags and packaging."""
import importlib.util
import json
import math
import os
import types

import pytest
import torch
import torch.nn.functional as F

import wloss_cases as wc

import dct_amd  # noqa: F401
from dct_amd.ckpt import build_checkpoint, save_checkpoint
from dct_amd.config import PipelineConfig, balanced_class_weight, default_config, parse_class_weight
from dct_amd.deploy.package import prepare_package
from dct_amd.models import build_model
from dct_amd.models.mlp import MLPClassifier, WeatherClassifier, build_mlp
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import confusion_weight_sum, weighted_infer_stats
from dct_amd.tracking import MlflowClient
from dct_amd.trainer import Trainer
from dct_amd.trainer import trainer as trainer_mod
from dct_amd.trainer.engines import FusedMLPEngine
from dct_amd.trainer.graph_engine import GraphMLPEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [wc.case_id(c) for c in wc.CASES]


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("variant", list(wc.VARIANTS))
@pytest.mark.parametrize("case", wc.CASES, ids=IDS)
def test_reference_equals_torch_cross_entropy_in_fp64(case, variant):
    dims, B = case
    w, eps = wc.variant_args(variant, dims[-1])
    for step in wc.grad_steps(case):
        ref = wc.reference(case, variant, step)
        z = ref["logits"].clone().requires_grad_()
        loss = F.cross_entropy(z, ref["y"], weight=None if w is None else w.double(), label_smoothing=eps)
        loss.backward()
        assert abs(ref["loss"] - loss.item()) <= 4 * 2.0 ** -53 * abs(loss.item())
        assert float((ref["dlogits"] - z.grad).abs().max()) < 1e-15
        # and the parameter gradient through the fp64 MLP
        p = wc.inputs(case)["p"].double().requires_grad_()
        x, y = wc.step_rows(case, step)
        F.cross_entropy(wc.forward64(dims, p, x), y, weight=None if w is None else w.double(),
                        label_smoothing=eps).backward()
        assert float((ref["grads"] - p.grad).abs().max()) < 1e-14


def test_inputs_are_discriminating():
    """Weights over [0.5, 4], every class in every tile that can hold them, W far from the row count."""
    for case in wc.CASES:
        dims, B = case
        C = dims[-1]
        w = wc.class_weights(C)
        assert float(w.min()) == 0.5 and float(w.max()) == 4.0 and len(w) == C
        d = wc.inputs(case)
        n = wc.n_items_of(B)
        assert len(d["idx"]) == n == len(set(d["idx"].tolist())) and wc.n_steps(B) == math.ceil(n / B) >= 3
        seq = d["Y"][d["idx"].long()].long()
        for first in range(0, n, B):
            bs = min(B, n - first)
            for r0 in range(0, bs, wc.R):
                live = min(wc.R, bs - r0)
                if live >= C:
                    assert set(seq[first + r0: first + r0 + live].tolist()) == set(range(C))
        for step in wc.grad_steps(case):
            ref = wc.reference(case, "w", step)
            assert abs(ref["W"] / len(ref["y"]) - 1.0) > 0.05


@pytest.mark.parametrize("mutant", wc.MUTANTS)
@pytest.mark.parametrize("case", wc.CASES, ids=IDS)
def test_mutants_fall_outside_the_gpu_tolerances(case, mutant):
    """On the very inputs of tests/test_wloss_gpu.py, with its grad-mode tolerances: each wrong implementation misses
    both the gradient check and the loss check, in every variant and step where it differs from the feature."""
    for variant in wc.MUTANT_VARIANTS[mutant]:
        for step in wc.grad_steps(case):
            ref = wc.reference(case, variant, step)
            bad = wc.reference(case, variant, step, mutant)
            g_ok, l_ok = wc.grads_inside(bad, ref)
            assert not g_ok and not l_ok, (variant, step)
    # where a mutant computes the feature itself it must of course pass: the reference agrees with itself
    ref = wc.reference(case, "ws", 0)
    assert wc.grads_inside(ref, ref) == (True, True)


@pytest.mark.parametrize("case", wc.CASES, ids=IDS)
def test_fp32_arithmetic_of_the_kernel_stays_inside_the_tolerances(case):
    """The row loss as csrc/mlp_fused_impl.h row_loss4_weighted writes it, in torch fp32 from fp32 logits, the fold's
    division by an fp32 W: inside the grad-mode tolerances on dlogits and loss (the conditions are reachable)."""
    dims, B = case
    C = dims[-1]
    for variant in wc.VARIANTS:
        w, eps = wc.variant_args(variant, C)
        w = torch.ones(C) if w is None else w
        for step in wc.grad_steps(case):
            ref = wc.reference(case, variant, step)
            z, y = ref["logits"].float(), ref["y"]
            mx = z.max(1, keepdim=True).values
            e = torch.exp(z - mx)
            s = e.sum(1, keepdim=True)
            lse = mx + torch.log(s)
            t = wc.target_mass(y, w, torch.tensor(eps, dtype=torch.float32), C)
            num = (t * (lse - z)).sum(1)
            dz = e * (t.sum(1, keepdim=True) / s) - t
            W = w[y].sum()
            assert torch.allclose((dz / W).double(), ref["dlogits"], atol=wc.GRAD_ATOL, rtol=wc.GRAD_RTOL)
            assert abs(float(num.sum() / W) - ref["loss"]) < wc.LOSS_ATOL


@pytest.mark.parametrize("case", wc.CASES, ids=IDS)
def test_w_from_the_confusion_matrix_is_exact(case):
    """The inference side keeps no accumulator for W: sum_c w[c] * (row sum c of the confusion matrix), in fp64 from
    the fp32 weights the device holds and the int64 counts, is sum_i w[y_i] to the last bit."""
    dims, B = case
    C = dims[-1]
    ref = wc.infer_reference(case, "ws")
    w32 = wc.class_weights(C)
    pred = torch.randint(0, C, ref["y"].shape, generator=torch.Generator().manual_seed(1))
    conf = torch.bincount(ref["y"] * C + pred, minlength=C * C).reshape(C, C)
    exact = math.fsum(float(w32[int(c)]) for c in ref["y"])
    assert confusion_weight_sum(conf, w32) == exact == ref["W"]
    assert confusion_weight_sum(conf, None) == float(ref["n"])
    mean, correct, conf2 = weighted_infer_stats(3.0, 7, conf, w32)
    assert mean == 3.0 / exact and correct == 7 and conf2 is conf
    assert math.isnan(weighted_infer_stats(0.0, 0, torch.zeros(C, C, dtype=torch.int64), w32)[0])


@pytest.mark.parametrize("case", wc.CASES, ids=IDS)
def test_inference_bound_is_tight_enough_to_see_the_mutants(case):
    """The bound on sum_i num_i is derived, not measured (worst-case rounding through the layers: up to 0.3 % of the
    sum at the widest shape); a dropped (1 - eps) or an unweighted smoothing term moves the sum by over ten times it."""
    ref = wc.infer_reference(case, "ws")
    assert 0 < ref["bound"] < 1e-2 * ref["num_sum"]
    dims, B = case
    d = wc.inputs(case)
    sel = d["idx"].long()
    z = wc.forward64(dims, d["p"].double(), d["X"][sel])
    w, eps = wc.variant_args("ws", dims[-1])
    for mutant in ("unweighted_smooth", "dropped_1m_eps"):
        bad = float(wc.row_terms(z, d["Y"][sel].long(), w.double(), eps, mutant)[0].sum())
        assert abs(bad - ref["num_sum"]) > 10 * ref["bound"]


# ------------------------------------------------------------------------------------------------ the model
def test_model_compute_loss_matches_torch():
    torch.manual_seed(0)
    x, y = torch.randn(33, 5), torch.randint(0, 3, (33,))
    m = MLPClassifier(5, hidden=(16,), num_classes=3, dropout=0.0, class_weight=[0.5, 2.0, 4.0], label_smoothing=0.1)
    z = m(x)
    want = F.cross_entropy(z, y, weight=torch.tensor([0.5, 2.0, 4.0]), label_smoothing=0.1)
    assert torch.equal(m.compute_loss(z, y), want)
    assert torch.equal(m.training_step((x, y), 0), want)
    plain = MLPClassifier(5, hidden=(16,), num_classes=3, dropout=0.0)
    assert torch.equal(plain.compute_loss(z, y), F.cross_entropy(z, y))
    assert "class_weight" not in m.state_dict() and list(m.state_dict()) == list(plain.state_dict())
    assert m.double().class_weight.dtype == torch.float64  # the buffer follows the module


@pytest.mark.parametrize("kw", [
    dict(class_weight=[1.0]), dict(class_weight=[1.0, 2.0, 3.0]), dict(class_weight=[1.0, 0.0]),
    dict(class_weight=[1.0, -2.0]), dict(class_weight=[1.0, float("nan")]), dict(class_weight=[1.0, float("inf")]),
    dict(label_smoothing=-0.1), dict(label_smoothing=1.0), dict(label_smoothing=float("nan")),
    dict(loss="mse", class_weight=[1.0, 2.0]), dict(loss="mse", label_smoothing=0.1)])
def test_bad_arguments_raise_value_error(kw):
    with pytest.raises(ValueError):
        MLPClassifier(5, **kw)
    if "loss" not in kw:
        with pytest.raises(ValueError):
            WeatherClassifier(5, **kw)


def test_fused_spec_and_hparams_carry_the_options_only_when_set():
    assert MLPClassifier(5).fused_spec() == {"dims": [5, 64, 2], "dropout": 0.2, "loss": "ce"}
    assert dict(MLPClassifier(5, hidden=(32,)).hparams) == {
        "input_dim": 5, "hidden": [32], "num_classes": 2, "dropout": 0.2, "loss": "ce", "lr": 0.01}
    m = MLPClassifier(5, class_weight=(1, 3), label_smoothing=0.1)
    spec = m.fused_spec()
    assert set(spec) == {"dims", "dropout", "loss", "class_weight", "label_smoothing"}
    assert torch.equal(spec["class_weight"], torch.tensor([1.0, 3.0])) and spec["label_smoothing"] == 0.1
    assert m.hparams["class_weight"] == [1.0, 3.0] and m.hparams["label_smoothing"] == 0.1
    assert set(MLPClassifier(5, label_smoothing=0.2).fused_spec()) == {"dims", "dropout", "loss", "label_smoothing"}
    assert dict(WeatherClassifier(5).hparams) == {"input_dim": 5}
    assert dict(WeatherClassifier(5, class_weight=[1.0, 3.0], label_smoothing=0.1).hparams) == {
        "input_dim": 5, "class_weight": [1.0, 3.0], "label_smoothing": 0.1}
    assert dict(WeatherClassifier(5, label_smoothing=0.1).hparams) == {"input_dim": 5, "label_smoothing": 0.1}
    for make in (lambda **kw: build_mlp("weather", 5, **kw), lambda **kw: build_model("weather", 5, **kw),
                 lambda **kw: build_model("weather-mlp-3x128", 5, lr=0.01, **kw)):
        b = make(class_weight=[1.0, 3.0], label_smoothing=0.1)
        assert b.class_weight.tolist() == [1.0, 3.0] and b.label_smoothing == 0.1
        assert make().class_weight is None and make().label_smoothing == 0.0
    json.dumps(dict(m.hparams))  # plain numbers: a checkpoint's hyper-parameters stay serialisable


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_reports_the_trainer_of_a_weighted_launch():
    nat = native()
    tile = nat.MlpPlan([5, 64, 2], 1024)
    assert tile.use_tile and tile.trainer(4, weighted=True) == "tile" and tile.trainer(4) == "tile"
    for b in (1, 17, 1024):
        assert tile.trainer(b, mode=1, weighted=True) == "tile"
    assert tile.trainer(1025, weighted=True) == "none"
    for bmax in (4, 16):
        plan = nat.MlpPlan([5, 64, 2], bmax)
        assert plan.trainer(4) != "none" and plan.trainer(4, weighted=True) == "none"
        assert nat.MlpPlan([5, 128, 128, 2], bmax).trainer(4, weighted=True) == "none"
    # a shape the batch-tiled trainer refuses (hidden width 256) has no weighted trainer on any plan
    assert not nat.mlp_tile_supported([5, 256, 2])
    assert nat.MlpPlan([5, 256, 2], 16).trainer(4, weighted=True) == "none"
    assert nat.MlpPlan([5, 256, 2], 1024).trainer(4, weighted=True) == "none"


# ------------------------------------------------------------------------------------------------ engine routing
class _Fake:
    def __init__(self, *a, **kw):
        self.kw = kw


def _routed(monkeypatch, model, engine, batch):
    """The class _make_engine picks on a (pretended) GPU, the engines replaced by recording stand-ins that keep the
    real ``applicable`` rules (which need no device)."""
    real = {"FusedMLPEngine": FusedMLPEngine, "GraphMLPEngine": GraphMLPEngine}
    for n in ("FusedMLPEngine", "GraphMLPEngine", "AutogradEngine"):
        ns = {"applicable": staticmethod(real[n].applicable)} if n in real else {}
        monkeypatch.setattr(trainer_mod, n, type(n, (_Fake,), ns))
    monkeypatch.delenv("DCT_ENGINE", raising=False)
    t = Trainer(accelerator="cpu", engine=engine, verbose=False)
    t.ctx = types.SimpleNamespace(device=torch.device("cuda", 0))
    model.to = lambda *a, **kw: model
    return type(t._make_engine(model, batch, 0)).__name__


def test_weighted_models_route_to_fused_or_autograd_never_to_graph(monkeypatch):
    wl = dict(class_weight=[1.0, 3.0], label_smoothing=0.1)
    narrow = lambda **kw: MLPClassifier(5, hidden=(64,), dropout=0.0, **kw)  # noqa: E731
    wide8 = lambda **kw: MLPClassifier(8, hidden=(64,), dropout=0.0, **kw)  # noqa: E731  (the graph engine's shape)
    big = lambda **kw: MLPClassifier(8, hidden=(256,), dropout=0.0, **kw)  # noqa: E731  (no tile trainer)
    for batch in (4, 16, 64, 1024):
        assert _routed(monkeypatch, narrow(**wl), "auto", batch) == "FusedMLPEngine"
        assert _routed(monkeypatch, wide8(**wl), "auto", batch) == "FusedMLPEngine"
        assert _routed(monkeypatch, big(**wl), "auto", batch) == "AutogradEngine"
        assert _routed(monkeypatch, narrow(label_smoothing=0.1), "auto", batch) == "FusedMLPEngine"
    assert _routed(monkeypatch, narrow(**wl), "auto", 2048) == "AutogradEngine"
    assert _routed(monkeypatch, narrow(**wl), "fused", 4) == "FusedMLPEngine"
    with pytest.raises(RuntimeError):
        _routed(monkeypatch, wide8(**wl), "graph", 64)
    with pytest.raises(RuntimeError):
        _routed(monkeypatch, big(**wl), "fused", 4)
    # without the options the routing is what it was
    assert _routed(monkeypatch, wide8(), "auto", 64) == "GraphMLPEngine"
    assert _routed(monkeypatch, big(), "auto", 64) == "GraphMLPEngine"
    assert _routed(monkeypatch, narrow(), "auto", 4) == "FusedMLPEngine"
    dev = torch.device("cuda", 0)
    assert not GraphMLPEngine.applicable(wide8(**wl), dev, 64) and GraphMLPEngine.applicable(wide8(), dev, 64)
    assert FusedMLPEngine.applicable(narrow(**wl), dev, 1) and not FusedMLPEngine.applicable(narrow(**wl), dev, 1025)
    assert not FusedMLPEngine.applicable(narrow(**wl), torch.device("cpu"), 4)


def test_weighted_model_trains_on_the_cpu_like_a_torch_loop():
    """The autograd engine needs nothing new: compute_loss is the loss."""
    from torch.utils.data import DataLoader

    from dct_amd.data.dataset import TensorPairDataset

    gen = torch.Generator().manual_seed(5)
    x = torch.randn(64, 5, generator=gen)
    y = (x[:, 0] > 0.8).long()
    torch.manual_seed(3)
    model = MLPClassifier(5, hidden=(16,), dropout=0.0, class_weight=[1.0, 3.0], label_smoothing=0.1)
    torch.manual_seed(3)
    twin = MLPClassifier(5, hidden=(16,), dropout=0.0)
    t = Trainer(max_epochs=1, accelerator="cpu", num_sanity_val_steps=0, logger=None, verbose=False)
    t.fit(model, DataLoader(TensorPairDataset(x, y), batch_size=16, shuffle=False))
    opt = torch.optim.Adam(twin.parameters(), lr=0.01)
    for s in range(4):
        opt.zero_grad()
        F.cross_entropy(twin(x[16 * s: 16 * s + 16]), y[16 * s: 16 * s + 16], weight=torch.tensor([1.0, 3.0]),
                        label_smoothing=0.1).backward()
        opt.step()
    for a, b in zip(model.parameters(), twin.parameters()):
        assert (a.detach().cpu() - b.detach()).abs().max() < 1e-5


# ------------------------------------------------------------------------------------------------ config and job
def test_balanced_weights_on_a_hand_counted_label_vector():
    y = torch.tensor([0, 0, 0, 0, 0, 0, 1, 1, 0, 0])  # 8 of class 0, 2 of class 1
    assert balanced_class_weight(y, 2) == [10 / (2 * 8), 10 / (2 * 2)]
    assert balanced_class_weight([0, 1, 2, 2], 3) == [4 / 3, 4 / 3, 4 / 6]
    with pytest.raises(ValueError, match="class"):
        balanced_class_weight([0, 0, 0], 2)
    with pytest.raises(ValueError):
        balanced_class_weight([0, 2], 2)
    assert parse_class_weight(None) is None and parse_class_weight("") is None
    assert parse_class_weight("balanced") == "balanced" and parse_class_weight("1, 3.5") == [1.0, 3.5]
    assert parse_class_weight((1, 2)) == [1.0, 2.0]
    with pytest.raises(ValueError):
        parse_class_weight("1,x")


def _job():
    spec = importlib.util.spec_from_file_location("train_ddp_job_wloss", os.path.join(ROOT, "jobs", "train_ddp.py"))
    job = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(job)
    return job


def test_config_keys_and_job_flags(tmp_path):
    cfg = default_config({})
    assert cfg.model.class_weight is None and cfg.model.label_smoothing == 0.0
    cfg = PipelineConfig.from_dict({"model": {"class_weight": [1.0, 3.0], "label_smoothing": 0.1}})
    assert list(cfg.model.class_weight) == [1.0, 3.0] and cfg.model.label_smoothing == 0.1
    assert PipelineConfig.from_dict({"model": {"class_weight": "balanced"}}).model.class_weight == "balanced"
    job = _job()
    a = job.parse_args([])
    assert a.class_weight is None and a.label_smoothing == 0.0
    a = job.parse_args(["--class-weight", "balanced", "--label-smoothing", "0.1"])
    assert a.class_weight == "balanced" and a.label_smoothing == 0.1
    # one epoch of the job itself on the CPU: the checkpoint records the balanced weights of the training split
    out = tmp_path / "models"
    argv = ["--synthetic-rows", "200", "--epochs", "1", "--accelerator", "cpu", "--no-mlflow", "--model-dir", str(out),
            "--class-weight", "balanced", "--label-smoothing", "0.1", "--batch-size", "16"]
    assert job.main(argv) == 0
    from dct_amd.ckpt.lightning_io import load_checkpoint
    from dct_amd.data.synthetic import weather_tensors
    from dct_amd.trainer import seed_everything

    hp = load_checkpoint(str(out / "last.ckpt"))["hyper_parameters"]
    assert hp["input_dim"] == 5 and hp["label_smoothing"] == 0.1
    seed_everything(42)
    _, y = weather_tensors(200, seed=0)
    split = torch.utils.data.random_split(range(200), [160, 40])[0]
    counts = torch.bincount(y[torch.as_tensor(split.indices)], minlength=2)
    assert hp["class_weight"] == pytest.approx([160 / (2 * int(c)) for c in counts])


# ------------------------------------------------------------------------------------------------ packaging
def test_weighted_checkpoint_packages_and_scores(tmp_path, monkeypatch):
    uri = "file://" + str(tmp_path / "mlruns")
    client = MlflowClient(uri)
    run = client.create_run(client.get_or_create_experiment("weather_forecasting")).run_id
    torch.manual_seed(1)
    model = WeatherClassifier(5, class_weight=[1.0, 3.0], label_smoothing=0.1)
    ck = tmp_path / "weather-best-epoch=00-val_loss=0.40.ckpt"
    save_checkpoint(build_checkpoint(model.state_dict(), epoch=0, global_step=10, hyper_parameters=dict(model.hparams)),
                    str(ck))
    client.log_batch(run, metrics=[{"key": "val_loss", "value": 0.4, "step": 1}])
    client.log_artifact(run, str(ck), "best_checkpoints")
    client.set_terminated(run)
    d = tmp_path / "deploy"
    info = prepare_package(str(d), tracking_uri=uri)
    assert info["run_id"] == run
    monkeypatch.setenv("AZUREML_MODEL_DIR", str(d))
    spec = importlib.util.spec_from_file_location("score_wloss", os.path.join(d, "score.py"))
    score = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(score)
    score.init()
    x = [[0.1, -0.2, 0.3, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0, 1.0]]
    out = score.run(json.dumps({"data": x}))
    model.eval()
    assert torch.allclose(torch.tensor(out["probabilities"]), torch.softmax(model(torch.tensor(x)), dim=1), atol=1e-6)
    # the template's plain-torch model takes the checkpoint's hyper-parameters as keywords
    plain = score.MODEL_CLASS(**dict(model.hparams))
    plain.load_state_dict(model.state_dict())
    # and the batch scoring job rebuilds the model from them
    spec = importlib.util.spec_from_file_location("score_batch_wloss", os.path.join(ROOT, "jobs", "score_batch.py"))
    job = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(job)
    rebuilt = job.model_from_checkpoint(str(ck))
    assert rebuilt.class_weight.tolist() == [1.0, 3.0] and rebuilt.label_smoothing == 0.1
