"""Class-weighted, label-smoothed cross-entropy on the GPU: the batch-tiled trainer (csrc/mlp_tile.hip) and the tiled
inference kernel (csrc/mlp_infer.hip) against the fp64 reference of tests/wloss_cases.py and torch.optim.Adam, the
launchers' refusals, Trainer.fit / validate on a weighted model and the DDP step path (run on a real MI355X).

The tolerances are test_mlp_tile_gpu.py's: its grad-mode check (atol 1e-6, rtol 1e-4 on the gradient, 1e-5 on the
loss) and its ``_check_against_torch`` thresholds, reimplemented here.  tests/test_wloss_cases_cpu.py shows that the
four wrong implementations (normalising by the row count, an unweighted smoothing term, W counting a tile's dead rows,
a dropped (1 - eps)) miss the grad-mode check on these very inputs."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, random_split

import infer_cases as ic
import wloss_cases as wc

import dct_amd  # noqa: F401
from dct_amd.data.dataset import TensorPairDataset, dataset_tensors
from dct_amd.data.synthetic import weather_tensors
from dct_amd.models.mlp import MLPClassifier
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params, weighted_infer_stats
from dct_amd.trainer import Trainer, seed_everything

pytestmark = pytest.mark.gpu
IDS = [wc.case_id(c) for c in wc.CASES]


@pytest.fixture(autouse=True)
def _fresh_knobs():
    native().reload_knobs()
    yield
    native().reload_knobs()


def _dev(case, cuda, k=2):
    d = wc.inputs(case, k)
    return d["X"].to(cuda), d["Y"].to(cuda), d["idx"].to(cuda)


def _wl(variant, C, cuda):
    w, eps = wc.variant_args(variant, C)
    return dict(class_weight=None if w is None else w.to(cuda), label_smoothing=eps)


# ------------------------------------------------------------------------------------------------ grad mode
@pytest.mark.parametrize("variant", list(wc.VARIANTS))
@pytest.mark.parametrize("case", wc.CASES, ids=IDS)
def test_grad_mode_matches_the_fp64_reference(case, variant, cuda):
    """One step: the full first batch, and the last batch of 5 rows (1 row at batch 4) whose other tiles are empty."""
    dims, B = case
    P = mlp_num_params(dims)
    X, Y, idx = _dev(case, cuda)
    n_items = wc.n_items_of(B)
    k = FusedMLPKernel(dims, bmax=1024)
    assert k.plan.use_tile and k.plan.trainer(B, mode=1, weighted=True) == "tile"
    p = wc.inputs(case)["p"].to(cuda)
    for step in wc.grad_steps(case):
        g = torch.full((P + 1,), 7.0, device=cuda)
        k.train(p, None, None, X, Y, idx[step * B:], n_items=n_items - step * B, batch=B, steps=1, t0=0, lr=0.01,
                grad_out=g, **_wl(variant, dims[-1], cuda))
        ref = wc.reference(case, variant, step)
        got = dict(grads=g[:P].cpu(), loss=g[P].item())
        print("step %d: grad excess over 1e-4|g|: %.3e, loss diff %.3e" % (
            step, (got["grads"].double() - ref["grads"]).abs().sub(wc.GRAD_RTOL * ref["grads"].abs()).max(),
            abs(got["loss"] - ref["loss"])))
        assert wc.grads_inside(got, ref) == (True, True)


# ------------------------------------------------------------------------------------------------ train mode
def _ref_net(dims, p):
    layers = []
    for i in range(len(dims) - 1):
        layers.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(torch.nn.ReLU())
    net = torch.nn.Sequential(*layers)
    with torch.no_grad():
        for lin, (W, b) in zip([l for l in net if isinstance(l, torch.nn.Linear)], ic.split_params(p, dims)):
            lin.weight.copy_(W)
            lin.bias.copy_(b)
    return net


def _flat(net):
    return torch.cat([t.detach().reshape(-1) for t in net.state_dict().values()])


def _torch_adam(net, X, Y, idx, B, steps, w, eps):
    opt = torch.optim.Adam(net.parameters(), lr=0.01)
    losses = []
    for s in range(steps):
        rows = idx[s * B:(s + 1) * B].long()
        opt.zero_grad()
        l = F.cross_entropy(net(X[rows]), Y[rows].long(), weight=w, label_smoothing=eps)
        l.backward()
        opt.step()
        losses.append(l.item())
    st = opt.state_dict()["state"]
    return (torch.tensor(losses), torch.cat([st[i]["exp_avg"].reshape(-1) for i in range(len(st))]),
            torch.cat([st[i]["exp_avg_sq"].reshape(-1) for i in range(len(st))]))


def _check_against_torch(p, m, v, losses, net, ref_losses, ref_m, ref_v):
    """test_mlp_tile_gpu.py::_check_against_torch's thresholds."""
    err = (p.cpu() - _flat(net)).abs()
    print("param err median %.3e max %.3e, loss err %.3e" % (err.median(), err.max(),
                                                             (losses.cpu() - ref_losses).abs().max()))
    assert err.median() < 1e-5, err.median()
    assert err.max() < 2e-3, err.max()
    assert torch.allclose(losses.cpu(), ref_losses, atol=2e-4, rtol=1e-3)
    if m is not None:
        assert torch.allclose(m.cpu(), ref_m, atol=1e-4, rtol=1e-2)
        assert torch.allclose(v.cpu(), ref_v, atol=1e-4, rtol=1e-2)


def _train(case, variant, cuda, calls=((0, 3), (3, 4))):
    dims, B = case
    d = wc.inputs(case, 6)
    X, Y, idx = _dev(case, cuda, 6)
    n_items = wc.n_items_of(B, 6)
    steps = wc.n_steps(B, 6)
    p = d["p"].to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(steps, device=cuda)
    k = FusedMLPKernel(dims, bmax=1024)
    for first, n in calls:
        k.train(p, m, v, X, Y, idx[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=first,
                step_base=first, lr=0.01, loss_out=losses[first:], **_wl(variant, dims[-1], cuda))
    torch.cuda.synchronize()
    return p, m, v, losses


@pytest.mark.parametrize("case", wc.CASES, ids=IDS)
def test_train_matches_torch_adam_on_the_weighted_smoothed_loss(case, cuda):
    """7 steps in two launches (3, then 4 at t0 = step_base = 3); the last batch has 5 rows."""
    dims, B = case
    d = wc.inputs(case, 6)
    steps = wc.n_steps(B, 6)
    assert steps == (7 if B > 5 else 8)
    p, m, v, losses = _train(case, "ws", cuda, ((0, 3), (3, steps - 3)))
    w, eps = wc.variant_args("ws", dims[-1])
    net = _ref_net(dims, d["p"])
    _check_against_torch(p, m, v, losses, net, *_torch_adam(net, d["X"], d["Y"], d["idx"], B, steps, w, eps))


def test_weighted_training_is_deterministic(cuda):
    """32 tiles per step: W and the gradients are folded in ascending tile index whatever order the tiles finished."""
    case = ([7, 48, 32, 3], 1024)
    a = _train(case, "ws", cuda)
    b = _train(case, "ws", cuda)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y)
    assert float(a[3].min()) > 0


# ------------------------------------------------------------------------------------------------ inference
@pytest.mark.parametrize("variant", list(wc.VARIANTS))
@pytest.mark.parametrize("case", wc.CASES, ids=IDS)
def test_infer_word0_is_the_weighted_numerator(case, variant, cuda):
    dims, B = case
    C = dims[-1]
    X, Y, idx = _dev(case, cuda)
    ref = wc.infer_reference(case, variant)
    n = ref["n"]
    k = FusedMLPKernel(dims, bmax=1024)
    p = wc.inputs(case)["p"].to(cuda)
    wl = _wl(variant, C, cuda)
    words = []
    for grid in (None, 1, 3):
        stats = torch.zeros(2 + C * C, dtype=torch.int64, device=cuda)
        pred = torch.zeros(n, dtype=torch.int32, device=cuda)
        k.infer(p, X, n, idx=idx, Y=Y, stats_out=stats, pred_out=pred, grid=grid, **wl)
        words.append(stats.cpu())
    assert torch.equal(words[0], words[1]) and torch.equal(words[0], words[2])  # word 0 included: the same bits
    num_sum, correct, conf = k.infer_stats(stats)
    print("sum num %.9f fp64 %.9f bound %.3e" % (num_sum, ref["num_sum"], ref["bound"]))
    assert abs(num_sum - ref["num_sum"]) <= ref["bound"]
    assert int(ref["ambiguous"].sum()) <= ic.MAX_AMBIGUOUS * n
    want_correct, want_conf = ic.expected_counts(ref, pred.cpu(), C)
    assert correct == want_correct and torch.equal(conf, want_conf)
    mean, _, _ = weighted_infer_stats(num_sum, correct, conf, wl["class_weight"])
    assert abs(mean - ref["num_sum"] / ref["W"]) <= ref["bound"] / ref["W"]
    # the unweighted launch is the plain CE sum it always was
    k.infer(p, X, n, idx=idx, Y=Y, stats_out=stats)
    d = wc.inputs(case)
    z, bz = ic.forward64(dims, d["p"], d["X"][d["idx"].long()])
    st = ic.stats64(z, bz, ref["y"], "ce")
    assert abs(k.infer_stats(stats)[0] - float(st["row_loss"].sum())) <= float(st["bound_loss"].sum())


# ------------------------------------------------------------------------------------------------ refusals
def test_launchers_refuse_bad_weighted_launches(cuda):
    case = wc.CASES[0]
    dims, B = case
    P = mlp_num_params(dims)
    X, Y, idx = _dev(case, cuda)
    p = wc.inputs(case)["p"].to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    g = torch.zeros(P + 1, device=cuda)
    stats = torch.zeros(6, dtype=torch.int64, device=cuda)
    w = torch.tensor([1.0, 3.0], device=cuda)
    tile = FusedMLPKernel(dims, bmax=1024)

    def train(k, **kw):
        k.train(p, m, v, X, Y, idx, n_items=B, batch=kw.pop("batch", B), steps=1, t0=0, lr=0.01, **kw)

    bad = [dict(class_weight=torch.ones(3, device=cuda)), dict(class_weight=torch.ones(1, device=cuda)),
           dict(class_weight=w.double()), dict(class_weight=w.cpu()), dict(class_weight=[1.0, 3.0]),
           dict(class_weight=w, loss="mse"), dict(label_smoothing=0.1, loss="mse"), dict(label_smoothing=1.0),
           dict(label_smoothing=-0.1)]
    for kw in bad:
        with pytest.raises(ValueError):
            train(tile, **kw)
        with pytest.raises(ValueError):
            train(tile, grad_out=g, **kw)
        with pytest.raises(ValueError):
            tile.infer(p, X, B, idx=idx, Y=Y, stats_out=stats, **kw)
    for bmax, batch in ((4, 4), (16, 4), (16, 16)):
        small = FusedMLPKernel(dims, bmax=bmax)
        assert small.plan.trainer(batch) != "none" and small.plan.trainer(batch, weighted=True) == "none"
        for kw in (dict(class_weight=w), dict(label_smoothing=0.1)):
            with pytest.raises(ValueError, match="batch-tiled"):
                train(small, batch=batch, **kw)
            with pytest.raises(ValueError, match="batch-tiled"):
                small.prepare_train(p, m, v, X, Y, idx, n_items=B, batch=batch, lr=0.01,
                                    step_counter=torch.zeros(1, dtype=torch.int32, device=cuda), **kw)
        # the native layer says the same to a caller that skips the Python checks
        with pytest.raises(ValueError, match="batch-tiled trainer's plan"):
            small.plan.train(p.data_ptr(), m.data_ptr(), v.data_ptr(), 0, X.data_ptr(), X.stride(0), Y.data_ptr(),
                             idx.data_ptr(), B, batch, 1, 0, 0.01, 0.9, 0.999, 1e-8, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0,
                             class_w=w.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), wc.inputs(case)["p"]) and not bool(m.any()) and not bool(g.any())  # nothing ran


# ------------------------------------------------------------------------------------------------ Trainer.fit
@pytest.mark.parametrize("B", [4, 64])
def test_trainer_fit_and_validate_on_a_weighted_model(B):
    """MLPClassifier(class_weight=[1, 3], label_smoothing=0.1) through Trainer.fit: the fused engine on the tile plan at
    batch 4 and at batch 64, the trajectory of a CPU torch loop, and val_loss = the whole shard's weighted mean."""
    w, eps = [1.0, 3.0], 0.1
    n_train, n_val = 10 * B - 1, 77
    seed_everything(42)
    x, y = weather_tensors(n_train + n_val, seed=0)
    tr, va = random_split(TensorPairDataset(x, y), [n_train, n_val])
    torch.manual_seed(0)
    model = MLPClassifier(5, (64,), class_weight=w, label_smoothing=eps, dropout=0)
    twin = copy.deepcopy(model)
    t = Trainer(max_epochs=1, accelerator="gpu", engine="auto", logger=None, num_sanity_val_steps=0, verbose=False)
    t.fit(model, DataLoader(tr, batch_size=B, shuffle=True), DataLoader(va, batch_size=B))
    eng = t.engine
    assert eng.name == "fused" and eng.weighted and eng.kernel.plan.use_tile
    assert eng.kernel.plan.trainer(B, weighted=True) == "tile"
    steps = math.ceil(n_train / B)
    assert steps == 10 and t.global_step == steps
    # the CPU torch loop over the engine's own batch order
    rows = eng.train_rows[eng.epoch_local_indices(n_train, 0, True)]
    opt = torch.optim.Adam(twin.parameters(), lr=0.01)
    ref_losses = []
    for s in range(steps):
        r = rows[s * B:(s + 1) * B]
        opt.zero_grad()
        l = F.cross_entropy(twin(x[r]), y[r], weight=torch.tensor(w), label_smoothing=eps)
        l.backward()
        opt.step()
        ref_losses.append(l.item())
    _check_against_torch(eng.p, None, None, eng._loss_buf[:steps], twin.net, torch.tensor(ref_losses), None, None)
    # validation: fit's and Trainer.validate's val_loss against fp64 on the trained weights
    p = eng.p.cpu()
    xv, yv = dataset_tensors(va)
    z, bz = ic.forward64([5, 64, 2], p, xv)
    w64 = torch.tensor(w, dtype=torch.float64)
    num, tm, _ = wc.row_terms(z, yv.long(), w64, eps)
    W = float(w64[yv.long()].sum())
    bound = torch.zeros_like(num)
    for c in range(2):
        bound += tm[:, c] * ic.stats64(z, bz, torch.full_like(yv.long(), c), "ce")["bound_loss"]
    bound = float((bound + 16 * ic.U * num.abs()).sum()) / W
    want = float(num.sum()) / W
    fit_loss = t.callback_metrics["val_loss"]
    out = t.validate()[0]
    print("val_loss fit %.9f validate %.9f fp64 %.9f bound %.3e" % (fit_loss, out["val_loss"], want, bound))
    assert abs(fit_loss - want) <= bound and abs(out["val_loss"] - want) <= bound
    # the confusion matrix: exact (rows whose fp64 top-2 gap is inside the logit bound may fall either way)
    top2 = z.topk(2, dim=1).values
    amb = (top2[:, 0] - top2[:, 1]) < 2 * bz.max(1).values
    conf = t.last_confusion_matrix
    assert int(amb.sum()) <= ic.MAX_AMBIGUOUS * n_val
    assert conf.dtype == torch.int64 and torch.equal(conf.sum(1), torch.bincount(yv.long(), minlength=2))
    hits = int((z.argmax(1) == yv)[~amb].sum())
    assert hits <= int(conf.diag().sum()) <= hits + int(amb.sum())
    assert int(conf.diag().sum()) == round(out["val_acc"] * n_val)
    if not bool(amb.any()):
        assert torch.equal(conf, ic.confusion(yv.long(), z.argmax(1), 2))


# ------------------------------------------------------------------------------------------------ DDP step path
@pytest.mark.parametrize("graph", ["1", "0"])
def test_weighted_ddp_step_path_world1_matches_persistent(graph, monkeypatch):
    """DCT_FORCE_DDP=1 at world size 1 (grad-mode tile launch pair with the weights -> one-rank all-reduce -> flat
    Adam, HIP-graph chunks of 7) reproduces the weighted train-mode launches; the tolerances of
    test_mlp_tile_gpu.py::test_tile_ddp_step_path_world1_matches_persistent."""
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import FusedMLPEngine, adam_hparams_from

    x, y = weather_tensors(3000, seed=1)
    rows = torch.randperm(3000, generator=torch.Generator().manual_seed(0))

    def run(force):
        monkeypatch.setenv("DCT_FORCE_DDP", force)
        monkeypatch.setenv("DCT_GRAPH", graph)
        monkeypatch.setattr(FusedMLPEngine, "GRAPH_CHUNK", 7)
        torch.manual_seed(0)
        model = MLPClassifier(5, hidden=(64,), dropout=0.0, class_weight=[1.0, 3.0], label_smoothing=0.1)
        ctx = init_distributed("gpu")
        eng = FusedMLPEngine(model, ctx, 48, seed=42, adam=adam_hparams_from(model.configure_optimizers()))
        assert eng.weighted and eng.kernel.plan.use_tile and not eng.fused_update and eng.xg is None
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
    # and it is the weighted loss that was trained: the unweighted persistent run ends somewhere else
    torch.manual_seed(0)
    plain = MLPClassifier(5, hidden=(64,), dropout=0.0)
    monkeypatch.setenv("DCT_FORCE_DDP", "0")
    eng = FusedMLPEngine(plain, init_distributed("gpu"), 48, seed=42,
                         adam=adam_hparams_from(plain.configure_optimizers()))
    eng.attach_data(x, y, rows[:2800], rows[2800:])
    loss = torch.zeros(64, device=eng.device)
    eng.run_steps(eng.upload_epoch_indices(0), 53, loss)
    torch.cuda.synchronize()
    assert (eng.p.cpu() - p0).abs().max() > 1e-2
