"""Trainer(accumulate_grad_batches=K) without a GPU: argument validation, engine routing (recording stand-ins), the
plan's answer for accumulating launches, and Trainer.fit on the autograd engine against a hand-written torch loop with
Lightning 2.1's semantics: the optimizer steps after batch b when (b + 1) % K == 0 or b is the epoch's last, on
(1 / K) * the sum of the window's micro-batch gradients - always 1 / K, also in a short last window - and global_step,
the logging cadence and a step-interval scheduler count optimizer steps."""
import math
import types

import pytest
import torch
import torch.nn.functional as F
import torch.optim.lr_scheduler as S
from torch.utils.data import DataLoader

import dct_amd  # noqa: F401
import dct_amd.trainer.trainer as trainer_mod
from dct_amd.data.dataset import TensorPairDataset
from dct_amd.data.synthetic import weather_tensors
from dct_amd.models.mlp import MLPClassifier
from dct_amd.ops._native import native
from dct_amd.tracking import InMemoryLogger
from dct_amd.trainer import Trainer
from dct_amd.trainer.engines import AutogradEngine, FusedMLPEngine

TOL = 1e-6  # tests/test_trainer_cpu.py's tolerance for a fit against its twin


# ------------------------------------------------------------------------------------------------ the argument
@pytest.mark.parametrize("k", [1, 2, 7])
def test_an_int_of_at_least_one_is_taken(k):
    assert Trainer(accelerator="cpu", verbose=False, accumulate_grad_batches=k).accumulate_grad_batches == k


def test_the_default_is_one():
    assert Trainer(accelerator="cpu", verbose=False).accumulate_grad_batches == 1


@pytest.mark.parametrize("k", [0, -1, 2.0, 1.5, True, False, None, "2", {0: 2}])
def test_anything_else_raises_value_error(k):
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        Trainer(accelerator="cpu", verbose=False, accumulate_grad_batches=k)
    for cls in (AutogradEngine, FusedMLPEngine):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            cls(MLPClassifier(5, dropout=0.0), types.SimpleNamespace(device=torch.device("cpu"), rank=0), 4, 0,
                **(dict(adam={}) if cls is FusedMLPEngine else {}), accumulate_grad_batches=k)


# ------------------------------------------------------------------------------------------------ routing
class _Fake:
    ok = True

    def __init__(self, *a, **kw):
        self.kw = kw

    @classmethod
    def applicable(cls, *a, **kw):
        cls.asked = a[3:]  # what follows (model, device, batch)
        return cls.ok


def _routed(monkeypatch, engine, batch, fused_ok=True, graph_ok=True, **kw):
    """The class _make_engine picks, with every engine replaced by a recording stand-in (no device needed)."""
    fakes = {n: type(n, (_Fake,), {}) for n in ("FusedMLPEngine", "GraphMLPEngine", "AutogradEngine")}
    fakes["FusedMLPEngine"].ok, fakes["GraphMLPEngine"].ok = fused_ok, graph_ok
    for n, c in fakes.items():
        monkeypatch.setattr(trainer_mod, n, c)
    monkeypatch.delenv("DCT_ENGINE", raising=False)
    t = Trainer(accelerator="cpu", engine=engine, verbose=False, **kw)
    t.ctx = types.SimpleNamespace(device=torch.device("cpu"))
    torch.manual_seed(0)
    e = t._make_engine(MLPClassifier(5, hidden=(64,), dropout=0.0), batch, 0)
    return type(e).__name__, e.kw, fakes


def test_the_keyword_reaches_an_engine_only_when_k_is_above_one(monkeypatch):
    for engine, fused_ok in (("auto", True), ("fused", True), ("auto", False), ("autograd", True)):
        name, kw, fakes = _routed(monkeypatch, engine, 4, fused_ok=fused_ok, graph_ok=False)
        assert "accumulate_grad_batches" not in kw
        assert fakes["FusedMLPEngine"].asked == ()  # applicable(model, device, batch), as before
        name1, kw1, _ = _routed(monkeypatch, engine, 4, fused_ok=fused_ok, graph_ok=False, accumulate_grad_batches=1)
        assert (name1, kw1) == (name, kw)
        name3, kw3, fakes = _routed(monkeypatch, engine, 4, fused_ok=fused_ok, graph_ok=False,
                                    accumulate_grad_batches=3)
        assert name3 == name and kw3 == dict(kw, accumulate_grad_batches=3)
        assert fakes["FusedMLPEngine"].asked == (3,)


def test_routing_with_accumulation(monkeypatch):
    # auto at batch 64: the fused engine although the graph engine would take the model - it does not accumulate
    assert _routed(monkeypatch, "auto", 64)[0] == "GraphMLPEngine"
    assert _routed(monkeypatch, "auto", 64, accumulate_grad_batches=2)[0] == "FusedMLPEngine"
    assert _routed(monkeypatch, "auto", 4, accumulate_grad_batches=2)[0] == "FusedMLPEngine"
    # not applicable: autograd, never the graph engine
    name, kw, _ = _routed(monkeypatch, "auto", 64, fused_ok=False, accumulate_grad_batches=2)
    assert name == "AutogradEngine" and kw["accumulate_grad_batches"] == 2
    with pytest.raises(RuntimeError, match="cannot accumulate"):
        _routed(monkeypatch, "graph", 64, accumulate_grad_batches=2)
    with pytest.raises(RuntimeError, match="not supported"):
        _routed(monkeypatch, "fused", 4, fused_ok=False, accumulate_grad_batches=2)
    assert _routed(monkeypatch, "graph", 64)[0] == "GraphMLPEngine"  # K = 1: as before
    # clipping still routes around the fused engine; with K > 1 that leaves autograd
    name, kw, _ = _routed(monkeypatch, "auto", 4, accumulate_grad_batches=2, gradient_clip_val=0.5)
    assert name == "AutogradEngine" and kw["gradient_clip_val"] == 0.5 and kw["accumulate_grad_batches"] == 2


def test_fused_engine_applicable_follows_the_tile_plan():
    dev = torch.device("cuda")  # (applicable only looks at the type)
    small, wide = MLPClassifier(5, hidden=(64,), dropout=0.0), MLPClassifier(5, hidden=(256,), dropout=0.0)
    assert FusedMLPEngine.applicable(small, dev, 4, 2) and FusedMLPEngine.applicable(small, dev, 256, 32)
    assert not FusedMLPEngine.applicable(small, dev, 256, 33)      # 33 * 8 slots
    assert not FusedMLPEngine.applicable(small, dev, 1025, 2)
    assert not FusedMLPEngine.applicable(wide, dev, 4, 2)          # not a tile shape
    assert not FusedMLPEngine.applicable(small, torch.device("cpu"), 4, 2)


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_names_the_trainer_of_an_accumulating_launch():
    nat = native()
    tile = nat.MlpPlan([5, 64, 2], 1024)
    assert nat.mlp_tile_max_slots() == 256
    for B in (1, 4, 16, 17, 40, 1024):
        assert tile.trainer(B) == tile.trainer(B, accumulate=1) == "tile"
        assert tile.trainer(B, accumulate=2) == tile.trainer(B, mode=1, cursor=True, accumulate=2) == "tile"
    # the slot cap: K * ceil(B / 32) <= 256
    assert tile.trainer(32, accumulate=256) == "tile" and tile.trainer(33, accumulate=128) == "tile"
    assert tile.trainer(32, accumulate=257) == "none" and tile.trainer(33, accumulate=129) == "none"
    assert tile.trainer(1024, accumulate=8) == "tile" and tile.trainer(1024, accumulate=9) == "none"
    assert tile.trainer(40, accumulate=2, world=2) == "none"       # no in-kernel exchange
    assert tile.trainer(40, mode=1, pending=True, accumulate=2) == "none"
    # every other plan refuses a window, at batches it otherwise takes
    for dims, bmax, B in (([5, 64, 2], 4, 4), ([5, 64, 2], 16, 16), ([5, 128, 128, 2], 4, 4),
                          ([5, 128, 128, 2], 16, 8), ([12, 40, 4], 16, 6), ([30, 128, 128, 3], 4, 3)):
        plan = nat.MlpPlan(dims, bmax)
        assert plan.trainer(B) != "none" and plan.trainer(B, accumulate=1) == plan.trainer(B)
        assert plan.trainer(B, accumulate=2) == "none"
        assert plan.trainer(B, mode=1, accumulate=2) == "none"
    assert nat.MlpPlan([5, 128, 128, 2], 4).trainer(4, world=2, accumulate=2) == "none"
    # and not only because the selector asks first: each of the other trainers' own predicates refuses the window
    b5, b3, wave = nat.MlpPlan([5, 128, 128, 2], 4), nat.MlpPlan([30, 128, 128, 3], 4), nat.MlpPlan([5, 64, 2], 4)
    for plan, which, kw in ((b5, "block5", dict(batch=4)), (b5, "block5", dict(batch=4, mode=1)),
                            (b5, "block5", dict(batch=4, world=2)), (b5, "block5_xg", dict(batch=4, world=2)),
                            (b3, "block3", dict(batch=3)), (b3, "block3", dict(batch=3, mode=1)),
                            (wave, "wave_rows", dict(batch=4)), (wave, "wave_xg", dict(batch=4, world=2))):
        assert plan.takes(which, **kw) and plan.takes(which, accumulate=1, **kw), (which, kw)
        assert not plan.takes(which, accumulate=2, **kw), (which, kw)
    assert nat.mlp_tile_window_ok(40, 128) and not nat.mlp_tile_window_ok(40, 129)
    assert nat.mlp_tile_window_ok(1024, 1) and not nat.mlp_tile_window_ok(1025, 1)
    # the workspace: K * T slots; the three-argument entry point is the K = 1 value
    one = nat.mlp_tile_ws_floats([5, 64, 2], 40)
    assert nat.mlp_tile_ws_floats_accum([5, 64, 2], 40, 1) == one
    assert nat.mlp_tile_ws_floats_accum([5, 64, 2], 40, 3) == 3 * (one - 4) + 4
    assert nat.mlp_tile_ws_floats_accum([5, 64, 2], 40, 129) == 0 and nat.mlp_tile_ws_floats_accum([5, 256, 2], 40, 2) == 0


# ------------------------------------------------------------------------------------------------ Trainer.fit
B, K, N, EPOCHS, EVERY = 4, 3, 42, 2, 3  # 11 batches (the last of 2 rows): windows of 3, 3, 3 and 2 batches


class _Scheduled(MLPClassifier):
    def __init__(self):
        super().__init__(5, hidden=(64,), dropout=0.0, lr=0.01)

    def configure_optimizers(self):
        opt = torch.optim.Adam(self.parameters(), lr=0.01)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": S.StepLR(opt, step_size=2, gamma=0.5),
                                                   "interval": "step"}}


def _model():
    torch.manual_seed(0)
    return _Scheduled()


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()


def _torch_loop(k):
    """Lightning's automatic optimization by hand: returns the parameters, the loss of every optimizer step's last
    micro-batch and the rate of every optimizer step."""
    x, y = weather_tensors(N, seed=0)
    model = _model()
    conf = model.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    nb = math.ceil(N / B)
    losses, rates = [], []
    for _ in range(EPOCHS):
        for b in range(nb):
            if b % k == 0:
                opt.zero_grad()
            loss = F.cross_entropy(model(x[b * B:(b + 1) * B]), y[b * B:(b + 1) * B])
            (loss / k).backward()
            if (b + 1) % k == 0 or b == nb - 1:
                rates.append(opt.param_groups[0]["lr"])
                opt.step()
                sched.step()
                losses.append(float(loss.detach()))
    return _flat(model), losses, rates


def _fit(k):
    x, y = weather_tensors(N, seed=0)
    model = _model()
    logger = InMemoryLogger()
    kw = dict(accumulate_grad_batches=k) if k != 1 else {}
    t = Trainer(max_epochs=EPOCHS, accelerator="cpu", engine="autograd", logger=logger, num_sanity_val_steps=0,
                verbose=False, enable_progress_bar=False, log_every_n_steps=EVERY, **kw)
    t.fit(model, DataLoader(TensorPairDataset(x, y), batch_size=B, shuffle=False),
          DataLoader(TensorPairDataset(x[:B], y[:B]), batch_size=B))
    return _flat(model), t, logger


def test_fit_is_the_hand_written_accumulation_loop():
    want, losses, rates = _torch_loop(K)
    got, t, logger = _fit(K)
    nb = math.ceil(N / B)
    steps = math.ceil(nb / K)
    assert nb % K != 0 and steps == 4 and len(losses) == EPOCHS * steps
    assert t.engine.name == "autograd" and t.engine.K == K
    err = float((got - want).abs().max())
    print("Trainer(accumulate_grad_batches=%d) vs the torch loop: max |dp| = %.3e" % (K, err))
    assert err < TOL
    # optimizer steps are the unit: global_step, Adam's count, the scheduler, the logging cadence
    assert t.global_step == t.engine.global_step == EPOCHS * steps
    assert t.engine.optimizer.step_count == EPOCHS * steps
    assert t.lr_schedule.scheduler.last_epoch == EPOCHS * steps
    assert t.lr_schedule.current_lr == pytest.approx(0.01 * 0.5 ** (EPOCHS * steps // 2))
    assert rates[-1] == pytest.approx(0.01 * 0.5 ** ((EPOCHS * steps - 1) // 2))
    hist = logger.history("train_loss")
    at = [s for s in range(EPOCHS * steps) if (s + 1) % EVERY == 0]
    assert [s for s, _ in hist] == at == [2, 5]
    assert [v for _, v in hist] == pytest.approx([losses[s] for s in at], abs=TOL)
    # and it is not K plain steps, nor the loop that divides a short window by its live batches
    plain, t1, _ = _fit(1)
    assert t1.global_step == EPOCHS * nb and float((plain - got).abs().max()) > 1000 * TOL


def test_k_one_is_the_plain_fit():
    a, ta, _ = _fit(1)
    want, _, _ = _torch_loop(1)
    assert float((a - want).abs().max()) < TOL and ta.engine.K == 1
