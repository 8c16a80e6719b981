"""Learning-rate schedulers on the CPU: the rate table LrSchedule fills from the user's torch scheduler against a plain
torch loop, Trainer.fit with a scheduler against a hand-written torch loop, checkpoints and resume, the rejected
configurations, and the LearningRateMonitor (trainer/lr_schedule.py, tests/lr_cases.py).

Tolerance of the torch-parity runs: max |dp| < 1e-6, the absolute tolerance tests/test_trainer_cpu.py compares two runs
of the same fit with.  The same fit with the scheduler removed differs from the scheduled one by more than 1000 times
that, so parity with the scheduled loop says something about the schedule."""
import warnings

import pytest
import torch
import torch.nn.functional as F
from torch.optim import lr_scheduler as S
from torch.utils.data import DataLoader

import dct_amd  # noqa: F401
import lr_cases as C
from dct_amd.ckpt import LearningRateMonitor, ModelCheckpoint, load_checkpoint
from dct_amd.data.dataset import TensorPairDataset
from dct_amd.data.synthetic import weather_tensors
from dct_amd.models.mlp import MLPClassifier
from dct_amd.tracking import InMemoryLogger
from dct_amd.trainer import Trainer
from dct_amd.trainer.lr_schedule import LrSchedule, parse_configure_optimizers

TOL = 1e-6
N_ROWS, B, EPOCHS = 48, 4, 3
STEPS = N_ROWS // B


# ---------------------------------------------------------------------------------------------- table filling
@pytest.mark.parametrize("interval,frequency", C.INTERVALS)
@pytest.mark.parametrize("name", list(C.SCHEDULERS))
def test_table_holds_the_rates_of_a_plain_torch_loop(name, interval, frequency):
    if name == "ReduceLROnPlateau" and interval == "step":
        with pytest.raises(ValueError, match="ReduceLROnPlateau"):
            opt = C.new_optimizer()
            LrSchedule(opt, C.SCHEDULERS[name](opt), interval, frequency, monitor="val_loss")
        return
    n_steps, epochs = 7, (6 if interval == "step" else 12)
    want = C.torch_rates(name, interval, frequency, n_steps, epochs)
    assert len({ep[0] for ep in want[1:]} | {want[0][0]}) >= 2, "the case does not vary the rate across epochs"
    opt = C.new_optimizer()
    sched = LrSchedule(opt, C.SCHEDULERS[name](opt), interval, frequency, monitor="val_loss")
    for e in range(epochs):
        t0 = 100 + e * n_steps  # (a resumed fit: the first window does not start at step 0)
        sched.begin_epoch(t0, n_steps)
        img = sched.table_image()
        rates = want[e] if interval == "step" else want[e][:1]
        assert torch.equal(img, C.table_image(t0, rates)), (e, img, C.table_image(t0, rates))
        assert int(img[0]) == t0 and int(img[1]) == len(rates) and int(img[2]) == int(img[3]) == 0
        # every step of the epoch reads its own rate (interval "epoch": one entry, every index clamps onto it), and
        # the clamp holds at both ends
        f32 = lambda x: float(torch.tensor(x, dtype=torch.float64).float())  # noqa: E731
        for b in range(n_steps):
            assert C.table_rate(img, t0 + b) == f32(want[e][b])
            assert sched.rate_for(t0 + b) == want[e][b]
        assert C.table_rate(img, t0 - 50) == C.table_rate(img, 0) == f32(want[e][0])
        assert C.table_rate(img, t0 + n_steps + 50) == f32(rates[-1])
        assert sched.rate_for(0) == want[e][0] and sched.rate_for(t0 + n_steps + 50) == rates[-1]
        sched.end_epoch(e, {"val_loss": C.PLATEAU_METRICS[e]})


def test_scheduler_step_warning_is_suppressed_not_avoided():
    opt = C.new_optimizer()
    sched = LrSchedule(opt, S.StepLR(opt, 1, 0.5), "step", 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sched.begin_epoch(0, 5)
        sched.end_epoch(0, {})
    assert sched.host == [C.BASE_LR * 0.5 ** k for k in range(5)]


# ---------------------------------------------------------------------------------------------- Trainer.fit
def _data():
    return weather_tensors(N_ROWS, seed=0)


class _Scheduled(MLPClassifier):
    """The 5-64-2 model; ``kind`` picks what configure_optimizers() returns."""

    def __init__(self, kind):
        super().__init__(5, hidden=(64,), dropout=0.0, lr=0.01)
        self.kind = kind

    def configure_optimizers(self):
        opt = torch.optim.Adam(self.parameters(), lr=0.01)
        if self.kind == "none":
            return opt
        if self.kind == "epoch":
            return {"optimizer": opt, "lr_scheduler": S.StepLR(opt, step_size=1, gamma=0.5)}
        if self.kind == "epoch_lists":
            return [opt], [S.StepLR(opt, step_size=1, gamma=0.5)]
        if self.kind == "warmup":
            return {"optimizer": opt, "lr_scheduler": {"scheduler": S.LinearLR(opt, start_factor=0.1, total_iters=10),
                                                       "interval": "step", "frequency": 1}}
        if self.kind == "sgd_warmup":
            opt = torch.optim.SGD(self.parameters(), lr=0.05, momentum=0.9)
            return {"optimizer": opt, "lr_scheduler": {"scheduler": S.LinearLR(opt, start_factor=0.1, total_iters=10),
                                                       "interval": "step"}}
        raise AssertionError(self.kind)


def _model(kind):
    torch.manual_seed(0)
    return _Scheduled(kind)


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()


def _torch_loop(kind, epochs=EPOCHS):
    """The hand-written loop: same data order, the optimizer and scheduler of configure_optimizers(), Lightning's
    stepping rules.  Returns the parameters and the rate of every step."""
    x, y = _data()
    model = _model(kind)
    conf = model.configure_optimizers()
    opt, cfg = parse_configure_optimizers(conf)
    sched = cfg["scheduler"] if cfg else None
    interval = cfg["interval"] if cfg else None
    rates = []
    for _ in range(epochs):
        for b in range(STEPS):
            opt.zero_grad()
            F.cross_entropy(model(x[b * B:(b + 1) * B]), y[b * B:(b + 1) * B]).backward()
            rates.append(opt.param_groups[0]["lr"])
            opt.step()
            if interval == "step":
                sched.step()
        if interval == "epoch":
            sched.step()
    return _flat(model), rates


def _fit(kind, epochs=EPOCHS, callbacks=None, logger=None, ckpt_path=None, log_every_n_steps=50):
    x, y = _data()
    model = _model(kind)
    t = Trainer(max_epochs=epochs, accelerator="cpu", engine="autograd", logger=logger, num_sanity_val_steps=0,
                verbose=False, enable_progress_bar=False, callbacks=callbacks, log_every_n_steps=log_every_n_steps)
    t.fit(model, DataLoader(TensorPairDataset(x, y), batch_size=B, shuffle=False),
          DataLoader(TensorPairDataset(x[:B], y[:B]), batch_size=B), ckpt_path=ckpt_path)
    return _flat(model), t


@pytest.mark.parametrize("kind", ["epoch", "epoch_lists", "warmup", "sgd_warmup"])
def test_trainer_fit_follows_the_scheduler_like_the_torch_loop(kind):
    """StepLR(step_size=1, gamma=0.5) per epoch (as a dict and as ([opt], [sched])), a step-interval warm-up, and the
    warm-up beside an optimizer that is not Adam (the real scheduler stepped in Python).  The run with the scheduler
    removed must differ: on the parent commit the scheduler is dropped and both runs are the same."""
    want, _ = _torch_loop(kind)
    got, t = _fit(kind)
    assert t.global_step == EPOCHS * STEPS and t.engine.name == "autograd"
    assert (t.engine.optimizer is None) == (kind == "sgd_warmup")
    err = float((got - want).abs().max())
    print("Trainer(%s) vs the scheduled torch loop: max |dp| = %.3e" % (kind, err))
    assert err < TOL
    if kind != "sgd_warmup":
        plain, _ = _fit("none")
        gap = float((got - plain).abs().max())
        print("  scheduled vs constant-rate fit: max |dp| = %.3e" % gap)
        assert gap > 1000 * TOL


def test_max_steps_advances_a_step_interval_scheduler_by_the_steps_that_ran():
    x, y = _data()
    model = _model("warmup")
    t = Trainer(max_epochs=2, max_steps=STEPS + 5, accelerator="cpu", engine="autograd", logger=None,
                num_sanity_val_steps=0, verbose=False)
    t.fit(model, DataLoader(TensorPairDataset(x, y), batch_size=B, shuffle=False),
          DataLoader(TensorPairDataset(x[:B], y[:B]), batch_size=B))
    assert t.global_step == STEPS + 5 and t.lr_schedule.scheduler.last_epoch == STEPS + 5
    x, y = _data()
    ref = _model("warmup")
    opt, cfg = parse_configure_optimizers(ref.configure_optimizers())
    for k in range(STEPS + 5):
        b = k % STEPS
        opt.zero_grad()
        F.cross_entropy(ref(x[b * B:(b + 1) * B]), y[b * B:(b + 1) * B]).backward()
        opt.step()
        cfg["scheduler"].step()
    assert float((_flat(model) - _flat(ref)).abs().max()) < TOL


# ---------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_carries_the_scheduler_and_resume_continues_it(tmp_path):
    saved = {}

    class Keep(ModelCheckpoint):  # keeps a copy of last.ckpt as it stood after epoch 1
        def on_validation_end(self, metrics, save_fn, is_rank_zero, epoch):
            out = super().on_validation_end(metrics, save_fn, is_rank_zero, epoch)
            if epoch == 1:
                saved["ckpt"] = load_checkpoint(str(tmp_path / "last.ckpt"))
                torch.save(saved["ckpt"], str(tmp_path / "epoch1.ckpt"))
            return out

    ck = Keep(dirpath=str(tmp_path), save_top_k=0, save_last=True)
    for kind in ("epoch", "warmup"):
        full, t = _fit(kind, callbacks=[ck])
        ckpt = saved["ckpt"]  # loaded by load_checkpoint: weights_only
        assert ckpt["epoch"] == 1 and len(ckpt["lr_schedulers"]) == 1
        # the scheduler state round-trips into a fresh scheduler, which then continues like the uninterrupted one
        _, rates = _torch_loop(kind)
        fresh = _model(kind)
        opt, cfg = parse_configure_optimizers(fresh.configure_optimizers())
        group = ckpt["optimizer_states"][0]["param_groups"][0]
        assert group["initial_lr"] == 0.01 and group["lr"] == pytest.approx(rates[2 * STEPS], rel=1e-12)
        opt.param_groups[0]["lr"] = group["lr"]
        cfg["scheduler"].load_state_dict(ckpt["lr_schedulers"][0])
        assert cfg["scheduler"].last_epoch == (2 if kind == "epoch" else 2 * STEPS)
        assert cfg["scheduler"].get_last_lr() == [pytest.approx(rates[2 * STEPS], rel=1e-12)]
        # resume after epoch 1: the uninterrupted run's parameters, exactly
        resumed, t2 = _fit(kind, ckpt_path=str(tmp_path / "epoch1.ckpt"))
        assert t2.global_step == EPOCHS * STEPS
        assert torch.equal(resumed, full), float((resumed - full).abs().max())


def test_checkpoint_without_a_scheduler_keeps_an_empty_list(tmp_path):
    ck = ModelCheckpoint(dirpath=str(tmp_path), save_top_k=0, save_last=True)
    _fit("none", epochs=1, callbacks=[ck])
    assert load_checkpoint(str(tmp_path / "last.ckpt"))["lr_schedulers"] == []


# ---------------------------------------------------------------------------------------------- rejected
def test_rejected_configurations_raise_the_documented_errors():
    opt = C.new_optimizer()
    with pytest.raises(ValueError, match="2 lr schedulers"):
        parse_configure_optimizers(([opt], [S.StepLR(opt, 1), S.ExponentialLR(opt, 0.9)]))
    with pytest.raises(ValueError, match="2 optimizers"):
        parse_configure_optimizers([opt, C.new_optimizer()])
    with pytest.raises(ValueError, match="needs 'monitor'"):
        LrSchedule.from_config(opt, parse_configure_optimizers(
            {"optimizer": opt, "lr_scheduler": S.ReduceLROnPlateau(opt)})[1])
    one = S.OneCycleLR(opt, max_lr=0.1, total_steps=10)  # cycle_momentum=True by default
    with pytest.raises(ValueError, match="cycle_momentum"):
        LrSchedule(opt, one, "step")
    ok = C.new_optimizer()
    LrSchedule(ok, S.OneCycleLR(ok, max_lr=0.1, total_steps=10, cycle_momentum=False), "step")  # (accepted)
    two = torch.optim.Adam([{"params": [torch.zeros(1, requires_grad=True)], "lr": 0.1},
                            {"params": [torch.zeros(1, requires_grad=True)], "lr": 0.2}])
    with pytest.raises(ValueError, match="different learning rates"):
        LrSchedule(two, S.StepLR(two, 1), "epoch")
    with pytest.raises(ValueError, match="interval"):
        LrSchedule(opt, S.StepLR(opt, 1), "batch")
    with pytest.raises(ValueError, match="unexpected keys"):
        parse_configure_optimizers({"optimizer": opt, "lr_scheduler": {"scheduler": S.StepLR(opt, 1), "every": 2}})


def test_plateau_reads_the_monitored_metric_after_validation():
    class Plateau(_Scheduled):
        def configure_optimizers(self):
            opt = torch.optim.Adam(self.parameters(), lr=0.01)
            # threshold 10: no validation loss ever counts as an improvement (the first included), so the rate halves
            # after every epoch's validation
            sched = S.ReduceLROnPlateau(opt, factor=0.5, patience=0, threshold=10.0)
            return {"optimizer": opt, "lr_scheduler": {"scheduler": sched, "monitor": "val_loss"}}

    torch.manual_seed(0)
    model = Plateau("plateau")
    x, y = _data()
    logger = InMemoryLogger()
    t = Trainer(max_epochs=3, accelerator="cpu", engine="autograd", logger=logger, num_sanity_val_steps=0,
                verbose=False, callbacks=[LearningRateMonitor()])
    t.fit(model, DataLoader(TensorPairDataset(x, y), batch_size=B, shuffle=False),
          DataLoader(TensorPairDataset(x[:B], y[:B]), batch_size=B))
    assert logger.history("lr-Adam") == [(0, 0.01), (STEPS, 0.005), (2 * STEPS, 0.0025)]
    assert t.lr_schedule.current_lr == 0.00125


def test_every_engine_is_handed_the_schedule(monkeypatch):
    """No engine fallback for a scheduler: the routing is what it is without one, and the engine gets the schedule."""
    import types

    from dct_amd.trainer import trainer as trainer_mod

    class Fake:
        ok = True

        def __init__(self, *a, **kw):
            self.kw = kw

        @classmethod
        def applicable(cls, *a, **kw):
            return cls.ok

    fakes = {n: type(n, (Fake,), {}) for n in ("FusedMLPEngine", "GraphMLPEngine", "AutogradEngine")}
    for n, c in fakes.items():
        monkeypatch.setattr(trainer_mod, n, c)
    monkeypatch.delenv("DCT_ENGINE", raising=False)
    for engine, batch, want in (("auto", 4, "FusedMLPEngine"), ("fused", 4, "FusedMLPEngine"),
                                ("auto", 64, "GraphMLPEngine"), ("autograd", 4, "AutogradEngine")):
        t = Trainer(accelerator="cpu", engine=engine, verbose=False)
        t.ctx = types.SimpleNamespace(device=torch.device("cpu"))
        e = t._make_engine(_model("warmup"), batch, 0)
        assert type(e).__name__ == want
        if want == "AutogradEngine":
            assert "optimizers" in e.kw
        else:
            assert isinstance(e.kw["lr_schedule"], LrSchedule) and e.kw["lr_schedule"].interval == "step"


# ---------------------------------------------------------------------------------------------- monitor
@pytest.mark.parametrize("kind,interval", [("epoch", None), ("warmup", None), ("warmup", "epoch"), ("epoch", "step"),
                                           ("sgd_warmup", "step")])
def test_learning_rate_monitor_logs_the_torch_loops_series(kind, interval):
    every = 5
    _, rates = _torch_loop(kind)
    logger = InMemoryLogger()
    _fit(kind, callbacks=[LearningRateMonitor(logging_interval=interval)], logger=logger, log_every_n_steps=every)
    per_step = (interval or ("step" if "warmup" in kind else "epoch")) == "step"
    if per_step:  # at the steps train_loss is logged at: every 5th optimizer step, step value k - 1
        want = [(k - 1, rates[k - 1]) for k in range(every, EPOCHS * STEPS + 1, every)]
        assert [s for s, _ in logger.history("train_loss")] == [s for s, _ in want]
    else:
        want = [(e * STEPS, rates[e * STEPS]) for e in range(EPOCHS)]
    got = logger.history("lr-SGD" if kind == "sgd_warmup" else "lr-Adam")
    assert got == want, (got, want)
