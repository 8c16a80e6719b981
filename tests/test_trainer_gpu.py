"""End-to-end training on the GPU engines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, random_split

import dct_amd  # noqa: F401
from dct_amd.ckpt import ModelCheckpoint, load_checkpoint
from dct_amd.data.dataset import TensorPairDataset
from dct_amd.data.synthetic import weather_tensors
from dct_amd.models.mlp import MLPClassifier, WeatherClassifier
from dct_amd.tracking import InMemoryLogger
from dct_amd.trainer import Trainer, seed_everything

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loaders(n=2000, bs=4):
    seed_everything(42)
    x, y = weather_tensors(n, seed=0)
    ds = TensorPairDataset(x, y)
    tr, va = random_split(ds, [int(0.8 * n), n - int(0.8 * n)])
    return DataLoader(tr, batch_size=bs, shuffle=True), DataLoader(va, batch_size=bs)


def test_fit_fused_engine_writes_lightning_checkpoints(tmp_path):
    tl, vl = _loaders()
    model = WeatherClassifier(5)
    ck = ModelCheckpoint(dirpath=str(tmp_path), filename="weather-best-{epoch:02d}-{val_loss:.2f}", monitor="val_loss",
                         mode="min", save_top_k=1, save_last=True)
    logger = InMemoryLogger()
    tr = Trainer(max_epochs=3, accelerator="gpu", logger=logger, callbacks=[ck], log_every_n_steps=5)
    tr.fit(model, tl, vl)
    assert tr.engine.name == "fused"
    assert os.path.exists(ck.best_model_path) and os.path.exists(tmp_path / "last.ckpt")
    ckpt = load_checkpoint(ck.best_model_path)
    assert set(ckpt["state_dict"]) == {"net.0.weight", "net.0.bias", "net.3.weight", "net.3.bias"}
    assert ckpt["hyper_parameters"] == {"input_dim": 5}
    m2 = WeatherClassifier.load_from_checkpoint(ck.best_model_path, input_dim=5)
    assert all(t.device.type == "cpu" for t in m2.state_dict().values())
    vals = [v for _, v in logger.history("val_loss")]
    assert len(vals) == 3 and vals[-1] < vals[0] + 0.05
    assert tr.callback_metrics["val_acc"] > 0.6
    # train_loss logged every 5 steps with step = k-1
    steps = [s for s, _ in logger.history("train_loss")]
    assert steps[:2] == [4, 9]


def test_fused_matches_autograd_engine_without_dropout():
    def run(engine, acc):
        tl, vl = _loaders(800)
        torch.manual_seed(0)
        model = MLPClassifier(5, hidden=(64,), dropout=0.0)
        tr = Trainer(max_epochs=2, accelerator=acc, engine=engine, num_sanity_val_steps=0, verbose=False)
        tr.fit(model, tl, vl)
        return tr.callback_metrics["val_loss"], model
    l_f, m_f = run("fused", "gpu")
    l_a, m_a = run("autograd", "cpu")
    assert abs(l_f - l_a) < 5e-3


def test_bench_contract_single_gpu(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "400", "--warmup", "40",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in out
    assert out["n_gpus"] == 1 and out["steps"] == 400 and out["value"] > 0
    assert out["extra"]["losses_finite"]
    # a plain run: no validation, measured epoch or reference model (those are --full)
    assert not {"val_loss", "epoch_wall_clock_s_measured", "reference_model_value"} & set(out["extra"])
    # --dump-outputs: the timed steps' losses and the state they left, float32
    n_params = 5 * 128 + 128 + 128 * 128 + 128 + 128 * 2 + 2
    for name, n in (("loss", 400), ("params", n_params), ("adam_m", n_params), ("adam_v", n_params)):
        x = np.load(os.path.join(str(tmp_path), name + ".npy"))
        assert x.dtype == np.float32 and x.shape == (n,) and np.isfinite(x).all(), name


@pytest.mark.parametrize("hidden", [(64,), (128, 128)])
@pytest.mark.parametrize("fused_update", ["1", "0"])
@pytest.mark.parametrize("graph", ["1", "0"])
def test_ddp_step_path_world1_matches_persistent(fused_update, graph, hidden, monkeypatch):
    """The DDP step loop (native RCCL comm, graph chunks, device cursor/step counter,
    update-then-grad) at world size 1 must reproduce the persistent single-launch path - for the
    reference 5-64-2 and for BASELINE's 3-layer 128-h MLP (grad-mode block kernel + flat Adam,
    the path its DDP=8 run takes)."""
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import FusedMLPEngine, adam_hparams_from

    x, y = weather_tensors(3000, seed=1)
    rows = torch.randperm(3000, generator=torch.Generator().manual_seed(0))

    def run(force):
        monkeypatch.setenv("DCT_FORCE_DDP", force)
        monkeypatch.setenv("DCT_GRAPH", graph)
        monkeypatch.setattr(FusedMLPEngine, "GRAPH_CHUNK", 7)
        monkeypatch.setattr(FusedMLPEngine, "FUSED_UPDATE", fused_update == "1")
        torch.manual_seed(0)
        model = MLPClassifier(5, hidden=hidden, dropout=0.0)
        ctx = init_distributed("gpu")
        eng = FusedMLPEngine(model, ctx, 4, seed=42, adam=adam_hparams_from(model.configure_optimizers()))
        eng.attach_data(x, y, rows[:2400], rows[2400:])
        n = eng.upload_epoch_indices(0)
        loss = torch.zeros(64, device=ctx.device)
        eng.run_steps(n, 30, loss, first_step=0)
        eng.run_steps(n, 23, loss, first_step=30)
        torch.cuda.synchronize()
        assert int(eng.step_counter.item()) == 53
        return eng.p.cpu(), eng.m.cpu(), loss[:53].cpu(), eng

    p0, m0, l0, _ = run("0")
    p1, m1, l1, e1 = run("1")
    assert e1.ddp and e1.comm is not None
    assert e1.graph_used == (graph == "1")
    # 3x128: the persistent kernel's Adam (step size folded into the denominator) and the flat Adam
    # kernel round differently - trajectories agree to fp32 noise, not bit for bit
    med = 1e-6 if hidden == (64,) else 1e-5
    assert torch.allclose(l0, l1, atol=1e-5 if hidden == (64,) else 1e-4), (l0 - l1).abs().max()
    assert (p0 - p1).abs().max() < 1e-3 and (p0 - p1).abs().median() < med
    assert torch.allclose(m0, m1, atol=1e-5 if hidden == (64,) else 1e-4)


def test_autograd_engine_logs_train_loss_after_graph_replays(monkeypatch):
    """From step GRAPH_WARMUP on the autograd engine replays its captured step graph, so
    training_step / self.log never run again: train_loss must still be logged every 5 steps and
    equal the eager run's values."""
    def run(graph: str):
        monkeypatch.setenv("DCT_GRAPH", graph)
        tl, vl = _loaders(400)
        torch.manual_seed(0)
        model = MLPClassifier(5, hidden=(64,), dropout=0.0)
        logger = InMemoryLogger()
        tr = Trainer(max_epochs=1, accelerator="gpu", engine="autograd", logger=logger, log_every_n_steps=5,
                     num_sanity_val_steps=0, verbose=False)
        tr.fit(model, tl, vl)
        assert tr.engine.name == "autograd" and tr.engine.graph_used == (graph == "1")
        return logger.history("train_loss"), tr.callback_metrics["train_loss"]

    hist_g, last_g = run("1")
    hist_e, last_e = run("0")
    steps = [s for s, _ in hist_g]
    assert steps == [s for s, _ in hist_e] == list(range(4, 80, 5))
    vg = torch.tensor([v for _, v in hist_g])
    ve = torch.tensor([v for _, v in hist_e])
    assert torch.isfinite(vg).all() and torch.allclose(vg, ve, atol=1e-4), (vg - ve).abs().max()
    assert abs(last_g - last_e) < 1e-4


def test_two_rank_trainer_on_one_gpu_in_kernel_exchange(tmp_path):
    """Two ranks sharing the GPU (gloo control plane): the Trainer picks the fused engine with the
    in-kernel exchange over IPC mappings; replicas stay bit-identical, rank 0 alone writes the
    checkpoints / MLflow run, and the exchange time is logged as allreduce_ms."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", "--master-port=29671", os.path.join(ROOT, "tests", "ddp_worker.py"),
           str(tmp_path), "2", "600", "gpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    p0 = json.loads((tmp_path / "params_rank0.json").read_text())
    p1 = json.loads((tmp_path / "params_rank1.json").read_text())
    assert p0["engine"] == "fused" and p0["xg"] and p0["params"] == p1["params"]
    exp = [d for d in os.listdir(tmp_path / "mlruns") if d.isdigit() and d != "0"][0]
    run = [d for d in os.listdir(tmp_path / "mlruns" / exp) if len(d) == 32][0]
    mdir = tmp_path / "mlruns" / exp / run / "metrics"
    assert {"train_loss", "val_loss", "allreduce_ms", "samples_per_sec"} <= set(os.listdir(mdir))
    ar = [float(ln.split()[1]) for ln in (mdir / "allreduce_ms").read_text().splitlines()]
    assert len(ar) == 2 and all(v > 0 for v in ar)
