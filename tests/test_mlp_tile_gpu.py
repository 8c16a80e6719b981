"""The batch-tiled fused trainer (csrc/mlp_tile.hip, per-rank batch 17..1024) against plain-torch fp32
references, the LDS trainer and the engines (run on a real MI355X)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, random_split

import dct_amd  # noqa: F401
from dct_amd.data.dataset import TensorPairDataset
from dct_amd.data.synthetic import weather_tensors
from dct_amd.models.mlp import MLPClassifier, WeatherClassifier
from dct_amd.ops._native import native, ptr, stream_handle
from dct_amd.ops.fused_mlp import FusedMLPKernel, dropout_keep_mask, mlp_num_params
from dct_amd.trainer import Trainer, seed_everything

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [([5, 64, 2], 17), ([5, 64, 2], 40), ([5, 128, 128, 2], 33), ([5, 128, 128, 2], 100), ([7, 48, 32, 3], 65),
          ([32, 128, 128, 4], 17)]


def _ref_net(dims):
    layers = []
    for i in range(len(dims) - 1):
        layers.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(torch.nn.ReLU())
    return torch.nn.Sequential(*layers)


def _flat(net):
    return torch.cat([t.detach().reshape(-1) for t in net.state_dict().values()])


def _ref_loss(logits, y, kind):
    if kind == "ce":
        return F.cross_entropy(logits, y)
    return F.mse_loss(logits, F.one_hot(y, logits.shape[1]).float())


@pytest.fixture(autouse=True)
def _fresh_knobs():
    """The native launchers read their DCT_* knobs at plan / bind time: every test starts from (and
    leaves) the environment as it is outside the test's monkeypatch."""
    native().reload_knobs()
    yield
    native().reload_knobs()


def _problem(dims, n_items, seed, cuda):
    torch.manual_seed(seed)
    N = n_items + 37
    X = torch.randn(N, dims[0])
    Y = torch.randint(0, dims[-1], (N,))
    idx = torch.randperm(N)[:n_items]
    net = _ref_net(dims)
    dev = (X.to(cuda), Y.to(cuda, torch.int32), idx.to(cuda, torch.int32))
    return X, Y, idx, net, dev


def _tile_train(k, p, m, v, dev, n_items, B, calls, losses, **kw):
    """``calls``: (first step, steps) launches over one index list, as the engine's chunks issue them."""
    Xd, Yd, idxd = dev
    for first, n in calls:
        k.train(p, m, v, Xd, Yd, idxd[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=first,
                step_base=first, lr=0.01, loss_out=losses[first:], **kw)
    torch.cuda.synchronize()


def _torch_adam(net, X, Y, idx, B, steps, loss, weight_decay=0.0, forward=None):
    opt = torch.optim.Adam(net.parameters(), lr=0.01, weight_decay=weight_decay)
    ref_losses = []
    for s in range(steps):
        rows = idx[s * B:(s + 1) * B]
        opt.zero_grad()
        out = net(X[rows]) if forward is None else forward(X[rows], s)
        l = _ref_loss(out, Y[rows], loss)
        l.backward()
        opt.step()
        ref_losses.append(l.item())
    st = opt.state_dict()["state"]
    ref_m = torch.cat([st[i]["exp_avg"].reshape(-1) for i in range(len(st))])
    ref_v = torch.cat([st[i]["exp_avg_sq"].reshape(-1) for i in range(len(st))])
    return torch.tensor(ref_losses), ref_m, ref_v


def _check_against_torch(p, m, v, losses, net, ref_losses, ref_m, ref_v):
    err = (p.cpu() - _flat(net)).abs()
    print("param err median %.3e max %.3e, loss err %.3e" % (err.median(), err.max(),
                                                             (losses.cpu() - ref_losses).abs().max()))
    assert err.median() < 1e-5, err.median()
    assert err.max() < 2e-3, err.max()
    assert torch.allclose(losses.cpu(), ref_losses, atol=2e-4, rtol=1e-3)
    assert torch.allclose(m.cpu(), ref_m, atol=1e-4, rtol=1e-2)
    assert torch.allclose(v.cpu(), ref_v, atol=1e-4, rtol=1e-2)


@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dims,B", SHAPES)
def test_tile_train_matches_torch_adam(dims, B, loss, cuda):
    """7 steps in two launches (3, then 4 at t0 = step_base = 3); the last batch has 5 rows, so whole
    tiles are empty there."""
    n_items = 6 * B + 5
    X, Y, idx, net, dev = _problem(dims, n_items, 1, cuda)
    p = _flat(net).to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    steps = math.ceil(n_items / B)
    assert steps == 7
    losses = torch.zeros(steps, device=cuda)
    k = FusedMLPKernel(dims, bmax=1024)
    assert k.plan.use_tile
    _tile_train(k, p, m, v, dev, n_items, B, ((0, 3), (3, 4)), losses, loss=loss)
    _check_against_torch(p, m, v, losses, net, *_torch_adam(net, X, Y, idx, B, steps, loss))


def _large_case(cuda):
    dims, B = [5, 128, 128, 2], 1024
    n_items = 2 * B + 5
    X, Y, idx, net, dev = _problem(dims, n_items, 5, cuda)
    return dims, B, n_items, X, Y, idx, net, dev


def _large_run(dims, B, n_items, net, dev, cuda):
    p = _flat(net).to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(3, device=cuda)
    k = FusedMLPKernel(dims, bmax=1024)
    _tile_train(k, p, m, v, dev, n_items, B, ((0, 3),), losses, loss="ce")
    return p, m, v, losses


def test_tile_train_batch_1024_matches_torch_adam(cuda):
    """32 tiles per step: workgroups on every XCD, folded across the kernel boundary."""
    dims, B, n_items, X, Y, idx, net, dev = _large_case(cuda)
    p, m, v, losses = _large_run(dims, B, n_items, net, dev, cuda)
    _check_against_torch(p, m, v, losses, net, *_torch_adam(net, X, Y, idx, B, 3, "ce"))


def test_tile_train_is_deterministic(cuda):
    """The slots are summed in ascending tile index whatever order the tiles finished in."""
    dims, B, n_items, X, Y, idx, net, dev = _large_case(cuda)
    a = _large_run(dims, B, n_items, net, dev, cuda)
    b = _large_run(dims, B, n_items, net, dev, cuda)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y)


@pytest.mark.parametrize("dims,B,n_items", [(d, b, b) for d, b in SHAPES] + [([5, 64, 2], 40, 37),
                                                                             ([5, 128, 128, 2], 40, 37)])
def test_tile_grad_mode_matches_autograd(dims, B, n_items, cuda):
    torch.manual_seed(2)
    N = 128
    X = torch.randn(N, dims[0])
    Y = torch.randint(0, dims[-1], (N,))
    idx = torch.arange(n_items, dtype=torch.int32)
    net = _ref_net(dims)
    p = _flat(net).to(cuda)
    P = mlp_num_params(dims)
    g = torch.zeros(P + 1, device=cuda)
    k = FusedMLPKernel(dims, bmax=1024)
    k.train(p, None, None, X.to(cuda), Y.to(cuda, torch.int32), idx.to(cuda), n_items=n_items, batch=B, steps=1, t0=0,
            lr=0.01, grad_out=g)
    l = F.cross_entropy(net(X[:n_items]), Y[:n_items])
    l.backward()
    want = torch.cat([q.grad.reshape(-1) for q in net.parameters()])
    got = g[:P].cpu()
    print("grad excess over 1e-4|g|: %.3e, loss diff %.3e" % ((got - want).abs().sub(1e-4 * want.abs()).max(),
                                                              abs(g[P].item() - l.item())))
    assert torch.allclose(got, want, atol=1e-6, rtol=1e-4)
    assert abs(g[P].item() - l.item()) < 1e-5


def test_tile_grad_mode_cursor_flushes_losses_and_advances(cuda):
    """The DDP step path's bookkeeping: the launch works at the device cursor, stores the previous
    step's grad_out[P] into loss_out[cursor - 1], and advances the cursor and the step counter."""
    dims, B, n_items = [5, 64, 2], 24, 60
    X, Y, idx, net, dev = _problem(dims, n_items, 3, cuda)
    p = _flat(net).to(cuda)
    P = mlp_num_params(dims)
    g = torch.zeros(P + 1, device=cuda)
    cursor = torch.zeros(1, dtype=torch.int32, device=cuda)
    counter = torch.full((1,), 9, dtype=torch.int32, device=cuda)
    losses = torch.zeros(3, device=cuda)
    k = FusedMLPKernel(dims, bmax=1024)
    want = []
    for s in range(3):
        k.train(p, None, None, *dev, n_items=n_items, batch=B, steps=1, t0=0, lr=0.01, grad_out=g, cursor=cursor,
                step_counter=counter, loss_out=losses)
        rows = idx[s * B:(s + 1) * B]
        want.append(F.cross_entropy(net(X[rows]), Y[rows]).item())
        assert abs(g[P].item() - want[-1]) < 1e-5
    assert int(cursor.item()) == 3 and int(counter.item()) == 12
    assert torch.allclose(losses[:2].cpu(), torch.tensor(want[:2]), atol=1e-5)
    assert losses[2].item() == 0.0  # flushed by the next launch (or by the engine at the end of a run)


@pytest.mark.parametrize("loss", ["ce", "mse"])
def test_tile_weight_decay_matches_torch_adam(loss, cuda):
    dims, B, n_items = [5, 128, 128, 2], 48, 48 * 6
    X, Y, idx, net, dev = _problem(dims, n_items, 6, cuda)
    p = _flat(net).to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(6, device=cuda)
    k = FusedMLPKernel(dims, bmax=1024)
    _tile_train(k, p, m, v, dev, n_items, B, ((0, 6),), losses, loss=loss, weight_decay=0.05)
    _torch_adam(net, X, Y, idx, B, 6, loss, weight_decay=0.05)
    err = (p.cpu() - _flat(net)).abs()
    assert err.median() < 1e-5, err.median()
    assert err.max() < 2e-3, err.max()


@pytest.mark.parametrize("dims,B", [([7, 128, 128, 2], 4), ([30, 128, 128, 3], 13), ([5, 64, 2], 16)])
def test_tile_kernel_draws_the_lds_kernels_dropout_mask(dims, B, cuda, monkeypatch):
    """DCT_MLP_BLOCK=tile forces the tile trainer at batch <= 16: same dropout hash, loss and Adam as the
    generic LDS trainer -> the same trajectory up to fp32 summation order."""
    torch.manual_seed(4)
    N, n_items = 500, 203
    X = torch.randn(N, dims[0]).to(cuda)
    Y = torch.randint(0, dims[-1], (N,)).to(cuda, torch.int32)
    idx = torch.randperm(N)[:n_items].to(cuda, torch.int32)
    p0 = _flat(_ref_net(dims)).to(cuda)
    steps = math.ceil(n_items / B)
    out = {}
    for name, kernel, block in (("tile", None, "tile"), ("lds", "lds", "0")):
        if kernel is None:
            monkeypatch.delenv("DCT_MLP_KERNEL", raising=False)
        else:
            monkeypatch.setenv("DCT_MLP_KERNEL", kernel)
        monkeypatch.setenv("DCT_MLP_BLOCK", block)
        native().reload_knobs()
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        losses = torch.zeros(steps, device=cuda)
        k = FusedMLPKernel(dims, bmax=4 if B <= 4 else 16)
        assert bool(k.plan.use_tile) == (name == "tile")
        k.train(p, m, v, X, Y, idx, n_items=n_items, batch=B, steps=steps, t0=3, lr=0.01, dropout=0.2, seed=11,
                step_base=5, loss_out=losses)
        torch.cuda.synchronize()
        out[name] = (p.cpu(), m.cpu(), v.cpu(), losses.cpu())
    monkeypatch.undo()
    for a_, b_ in zip(out["tile"], out["lds"]):
        assert torch.isfinite(a_).all()
        assert (a_ - b_).abs().max() <= 1e-4 * (1 + b_.abs().max()), float((a_ - b_).abs().max())


def test_tile_dropout_above_row_63_matches_host_mask(cuda):
    """Rows >= 64 fold b >> 6 into the hash: the trajectory equals torch Adam under the host mirror's mask."""
    dims, B, pdrop, seed = [5, 128, 128, 2], 100, 0.2, 11
    n_items = 7 * B
    X, Y, idx, net, dev = _problem(dims, n_items, 8, cuda)
    p = _flat(net).to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(7, device=cuda)
    k = FusedMLPKernel(dims, bmax=1024)
    _tile_train(k, p, m, v, dev, n_items, B, ((0, 7),), losses, loss="ce", dropout=pdrop, seed=seed)
    scale = (torch.ones((), dtype=torch.float32) / (torch.ones((), dtype=torch.float32) - torch.tensor(
        pdrop, dtype=torch.float32)))
    lins = [l for l in net if isinstance(l, torch.nn.Linear)]

    def forward(x, s):
        h = x
        for li, lin in enumerate(lins[:-1]):
            keep = dropout_keep_mask(seed, s, li, x.shape[0], lin.out_features, pdrop)
            h = torch.relu(lin(h)) * keep * scale
        return lins[-1](h)

    _check_against_torch(p, m, v, losses, net, *_torch_adam(net, X, Y, idx, B, 7, "ce", forward=forward))


@pytest.mark.parametrize("dims", [[5, 128, 128, 2], [5, 64, 2]])
def test_tile_train_refuses_a_parameter_pointer_off_the_16_byte_boundary(dims, cuda):
    """W1 is read as float4 at p + woff[1]: a contiguous view one float into an aligned allocation passes the Python
    checks, and both tiled launchers (one host check, csrc/mlp_tile_fwd.h) refuse it before any launch - nothing is
    written.  The aligned view of the same allocation goes through."""
    B, poison = 33, 12345.0
    X, Y, idx, net, dev = _problem(dims, B, 9, cuda)
    P = mlp_num_params(dims)
    k = FusedMLPKernel(dims, bmax=1024)
    assert k.plan.trainer(B) == "tile"
    buf = torch.zeros(P + 1, device=cuda)
    assert buf.data_ptr() % 16 == 0
    m, v = torch.full((P,), poison, device=cuda), torch.full((P,), poison, device=cuda)
    losses = torch.full((1,), poison, device=cuda)
    logits = torch.full((B, dims[-1]), poison, device=cuda)
    p = buf[1:P + 1]
    p.copy_(_flat(net))
    with pytest.raises(RuntimeError, match="invalid"):
        _tile_train(k, p, m, v, dev, B, B, ((0, 1),), losses)
    with pytest.raises(RuntimeError, match="invalid"):
        native().mlp_infer(dims, ptr(p), ptr(dev[0]), dev[0].stride(0), 0, 0, B, 0, 0, 0, ptr(logits), 0, 0, 0, 0, 0, 0,
                           stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), _flat(net))
    for t in (m, v, losses, logits):
        assert bool((t == poison).all())
    p = buf[:P]
    p.copy_(_flat(net))
    m.zero_(), v.zero_()
    _tile_train(k, p, m, v, dev, B, B, ((0, 1),), losses)
    assert math.isfinite(losses.item()) and losses.item() != poison
    assert bool(torch.isfinite(p).all()) and not torch.equal(p.cpu(), _flat(net))


def _loaders(n=2000, bs=64):
    seed_everything(42)
    x, y = weather_tensors(n, seed=0)
    ds = TensorPairDataset(x, y)
    tr, va = random_split(ds, [int(0.8 * n), n - int(0.8 * n)])
    return DataLoader(tr, batch_size=bs, shuffle=True), DataLoader(va, batch_size=bs)


def test_trainer_picks_the_tile_path_at_batch_64():
    tl, vl = _loaders()
    tr = Trainer(max_epochs=2, accelerator="gpu", engine="auto", num_sanity_val_steps=0, verbose=False)
    tr.fit(WeatherClassifier(5), tl, vl)
    assert tr.engine.name == "fused" and tr.engine.kernel.plan.use_tile
    assert math.isfinite(tr.callback_metrics["val_loss"])


def test_trainer_engine_choice_and_numerics_at_batch_64():
    def fit(make, engine, acc="gpu", epochs=1, feats=5):
        seed_everything(42)
        x, y = weather_tensors(2000, seed=0)
        if feats != x.shape[1]:
            x = torch.cat([x, x[:, : feats - x.shape[1]]], dim=1)
        ds = TensorPairDataset(x, y)
        tr_ds, va_ds = random_split(ds, [1600, 400])
        tl, vl = DataLoader(tr_ds, batch_size=64, shuffle=True), DataLoader(va_ds, batch_size=64)
        torch.manual_seed(0)
        model = make()
        tr = Trainer(max_epochs=epochs, accelerator=acc, engine=engine, num_sanity_val_steps=0, verbose=False)
        tr.fit(model, tl, vl)
        return tr

    wide = lambda: MLPClassifier(8, hidden=(64,), dropout=0.0)  # noqa: E731
    assert fit(wide, "auto", feats=8).engine.name == "graph"
    assert fit(wide, "fused", feats=8).engine.name == "fused"
    narrow = lambda: MLPClassifier(5, hidden=(64,), dropout=0.0)  # noqa: E731
    t_f = fit(narrow, "fused", "gpu", 2)
    assert t_f.engine.name == "fused" and t_f.engine.kernel.plan.use_tile
    t_a = fit(narrow, "autograd", "cpu", 2)
    assert abs(t_f.callback_metrics["val_loss"] - t_a.callback_metrics["val_loss"]) < 5e-3


@pytest.mark.parametrize("hidden", [(64,), (128, 128)])
@pytest.mark.parametrize("graph", ["1", "0"])
def test_tile_ddp_step_path_world1_matches_persistent(graph, hidden, monkeypatch):
    """The DDP step loop at batch 48 (grad-mode tile launch pair -> one-rank RCCL all-reduce -> flat
    Adam, HIP-graph chunks of 7, device cursor / step counter) reproduces the train-mode launches."""
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import FusedMLPEngine, adam_hparams_from

    x, y = weather_tensors(3000, seed=1)
    rows = torch.randperm(3000, generator=torch.Generator().manual_seed(0))

    def run(force):
        monkeypatch.setenv("DCT_FORCE_DDP", force)
        monkeypatch.setenv("DCT_GRAPH", graph)
        monkeypatch.setattr(FusedMLPEngine, "GRAPH_CHUNK", 7)
        torch.manual_seed(0)
        model = MLPClassifier(5, hidden=hidden, dropout=0.0)
        ctx = init_distributed("gpu")
        eng = FusedMLPEngine(model, ctx, 48, seed=42, adam=adam_hparams_from(model.configure_optimizers()))
        assert eng.kernel.plan.use_tile and not eng.fused_update and eng.xg is None
        eng.attach_data(x, y, rows[:2800], rows[2800:])
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
    assert torch.allclose(l0, l1, atol=1e-4), (l0 - l1).abs().max()
    assert (p0 - p1).abs().max() < 1e-3 and (p0 - p1).abs().median() < 1e-5
    assert torch.allclose(m0, m1, atol=1e-4)


def test_bench_runs_weather_3x128_at_batch_256():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--model", "weather-mlp-3x128", "--batch",
                        "256", "--steps", "200", "--warmup", "20"], capture_output=True, text=True, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["value"] > 0
    assert out["extra"]["losses_finite"]
