"""AdamW and SGD on the GPU (run on a real MI355X): the batch-tiled trainer's fold (csrc/mlp_tile.hip,
MlpArgs::opt_kind) and the flat SGD step (csrc/optim.hip) element by element against the fp64 reference and the derived
bound of tests/optim_cases.py, seven steps against torch.optim.SGD / AdamW, the refusals, Trainer.fit on the fused
engine, the checkpoint round trip and the DDP step path.

tests/test_optim_cases_cpu.py shows that the nine wrong implementations miss the bound on these very inputs; the
trajectory thresholds are test_accum_gpu.py::_check_against_torch's, set for 7 Adam steps (SGD has no division and sits
well inside them: the one-step test carries the discrimination)."""
import math

import pytest
import torch
import torch.nn.functional as F
import torch.optim.lr_scheduler as S
from torch.utils.data import DataLoader, random_split

import accum_cases as ac
import infer_cases as ic
import lr_cases as L
import optim_cases as oc
import wloss_cases as wc

import dct_amd  # noqa: F401
from dct_amd.data.dataset import TensorPairDataset
from dct_amd.data.synthetic import weather_tensors
from dct_amd.models.mlp import MLPClassifier
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params
from dct_amd.ops.optim import sgd_flat_
from dct_amd.trainer import Trainer, seed_everything

pytestmark = pytest.mark.gpu
IDS = [oc.case_id(c) for c in oc.CASES]
SEED, DROPOUT = 11, 0.1


@pytest.fixture(autouse=True)
def _fresh_knobs():
    native().reload_knobs()
    yield
    native().reload_knobs()


def _dev(d, cuda):
    return d["X"].to(cuda), d["Y"].to(cuda), d["idx"].to(cuda)


def _table(taken, cuda):
    """A rate table whose entry for ``taken`` steps taken is optim_cases.LR, between two rates that are far off."""
    return L.table_image(taken - 1, [0.5, oc.LR, 0.7]).to(cuda).view(torch.float32)


def _moments(hp, m, v, cuda):
    """What a launch binds: m and v for AdamW, the buffer alone for SGD, nothing without momentum."""
    if hp.kind == "sgd":
        return (m.to(cuda) if hp.momentum else None), None
    return m.to(cuda), v.to(cuda)


def _one_step(k, case, hp, taken, d, cuda, off=0, table=False, **extra):
    """A grad-mode launch and a train-mode launch from the same state, seed and step word (so: the same dropout masks):
    (got p / m / v on the CPU, the reference applied to the kernel's own folded gradient, both loss words)."""
    dims, B = case
    P = mlp_num_params(dims)
    X, Y, idx = _dev(d, cuda)
    n_items = d["idx"].numel() - off
    p0, m0, v0 = oc.state(case, hp, taken)
    common = dict(n_items=n_items, batch=B, steps=1, t0=taken, step_base=taken, dropout=DROPOUT, seed=SEED, **extra)
    g = torch.full((P + 1,), 7.0, device=cuda)
    k.train(p0.to(cuda), None, None, X, Y, idx[off:], lr=oc.LR, grad_out=g, **common)
    p = p0.to(cuda)
    m, v = _moments(hp, m0, v0, cuda)
    loss = torch.zeros(1, device=cuda)
    k.train(p, m, v, X, Y, idx[off:], lr=oc.LR_BASE if table else oc.LR, lr_tab=_table(taken, cuda) if table else None,
            loss_out=loss, **oc.kernel_args(hp), **common)
    torch.cuda.synchronize()
    ref = oc.reference(p0, g[:P].cpu(), m0, v0, hp, taken)
    got = (p.cpu(), None if m is None else m.cpu(), None if v is None else v.cpu())
    return got, ref, float(loss.item()), float(g[P].item())


# ------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("variant", list(oc.VARIANTS))
@pytest.mark.parametrize("case", oc.CASES, ids=IDS)
def test_one_step_lies_inside_the_derived_bound(case, variant, cuda):
    """Every step count, with the scalar rate and with the rate read from a table (the scalar then three times too
    large).  The fold computes the gradient word the same way in grad and in train mode, so the reference applied to
    the grad-mode launch's fp32 gradient isolates the optimizer arithmetic; the loss words are equal."""
    dims, B = case
    hp = oc.VARIANTS[variant]
    d = wc.inputs((dims, B))
    k = FusedMLPKernel(dims, bmax=1024)
    assert k.plan.trainer(B, optimizer=hp.kind) == "tile"
    for taken in oc.STEP_COUNTS:
        for table in (False, True):
            got, ref, loss, gloss = _one_step(k, case, hp, taken, d, cuda, table=table)
            print("%s %s t=%d table=%d: worst |error| / bound %.4f" % (oc.case_id(case), variant, taken, table,
                                                                     oc.excess(got, ref)))
            assert oc.inside(got, ref)
            assert loss == gloss and loss > 0


@pytest.mark.parametrize("variant", ["sgd_nest", "adamw"])
def test_one_step_with_weighted_loss_and_accumulation(variant, cuda):
    """The optimizer is orthogonal to how the gradient was folded: class weights + smoothing, windows of K = 3
    micro-batches (the full first window and the short last one), and both together."""
    dims, B, K = acase = ac.CASES[1]
    case, hp = (dims, B), oc.VARIANTS[variant]
    w, eps = ac.variant_args("ws", dims[-1])
    wl = dict(class_weight=w.to(cuda), label_smoothing=eps)
    k = FusedMLPKernel(dims, bmax=1024)
    for extra, d, offs in ((wl, wc.inputs(case), (0, 2 * B)),
                           (dict(accumulate=K), ac.inputs(acase), [win * K * B for win in ac.windows(acase)]),
                           (dict(accumulate=K, **wl), ac.inputs(acase), [win * K * B for win in ac.windows(acase)])):
        for off in offs:
            for taken in oc.STEP_COUNTS:
                got, ref, loss, gloss = _one_step(k, case, hp, taken, d, cuda, off=off, table=taken == 3, **extra)
                print("%s %s off=%d t=%d: worst |error| / bound %.4f" % (variant, sorted(extra), off, taken,
                                                                        oc.excess(got, ref)))
                assert oc.inside(got, ref) and loss == gloss and loss > 0


# ------------------------------------------------------------------------------------------------ seven steps
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


STEPS = 7


def _train(case, hp, cuda, calls=((0, 3), (3, 4)), pass_optimizer=True):
    dims, B = case
    # 6 full batches and 5 rows: 7 steps (at B = 4 the 5 rows are a batch and a row: 5 full batches before them)
    d = wc.inputs(case, 6 if B > 5 else 5)
    n_items = d["idx"].numel()
    assert math.ceil(n_items / B) == STEPS
    X, Y, idx = _dev(d, cuda)
    p = d["p"].to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    bm, bv = (m, v) if hp is None else _moments(hp, m, v, cuda)
    losses = torch.zeros(STEPS, device=cuda)
    k = FusedMLPKernel(dims, bmax=1024)
    kw = {} if hp is None else oc.kernel_args(hp)
    if hp is None and pass_optimizer:
        kw = dict(optimizer="adam")
    for first, n in calls:
        k.train(p, bm, bv, X, Y, idx[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=first,
                step_base=first, lr=oc.LR, loss_out=losses[first:], seed=SEED, **kw)
    torch.cuda.synchronize()
    return p, bm, bv, losses, d


@pytest.mark.parametrize("variant", list(oc.VARIANTS))
@pytest.mark.parametrize("case", oc.CASES, ids=IDS)
def test_seven_steps_match_torch(case, variant, cuda):
    """7 steps in two launches (3, then 4 at t0 = step_base = 3) against torch's optimizer on a CPU fp32 copy of the
    net; momentum_buffer plays m."""
    dims, B = case
    hp = oc.VARIANTS[variant]
    p, m, v, losses, d = _train(case, hp, cuda)
    net = _ref_net(dims, d["p"])
    opt = oc.torch_optimizer(net.parameters(), hp, dtype_exact=False)
    ref_losses = []
    for s in range(STEPS):
        rows = d["idx"][s * B:(s + 1) * B].long()
        opt.zero_grad()
        l = F.cross_entropy(net(d["X"][rows]), d["Y"][rows].long())
        l.backward()
        opt.step()
        ref_losses.append(l.item())
    err = (p.cpu() - _flat(net)).abs()
    lerr = (losses.cpu() - torch.tensor(ref_losses)).abs().max()
    print("%s %s: param err median %.3e max %.3e, loss err %.3e" % (oc.case_id(case), variant, err.median(), err.max(),
                                                                    lerr))
    assert err.median() < 1e-5, err.median()
    assert err.max() < 2e-3, err.max()
    assert torch.allclose(losses.cpu(), torch.tensor(ref_losses), atol=2e-4, rtol=1e-3)
    st = [opt.state[q] for q in net.parameters()]
    if m is not None:
        key = "momentum_buffer" if hp.kind == "sgd" else "exp_avg"
        assert torch.allclose(m.cpu(), torch.cat([s[key].reshape(-1) for s in st]), atol=1e-4, rtol=1e-2)
    if v is not None:
        assert torch.allclose(v.cpu(), torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]), atol=1e-4, rtol=1e-2)


def test_optimizer_adam_is_bit_identical_to_not_passing_it(cuda):
    for case in (([5, 64, 2], 40), ([7, 48, 32, 3], 65)):
        a = _train(case, None, cuda, pass_optimizer=False)
        b = _train(case, None, cuda, pass_optimizer=True)
        for x, y in zip(a[:4], b[:4]):
            assert torch.isfinite(x).all() and torch.equal(x, y)
        assert bool(a[1].any()) and bool(a[2].any())


# ------------------------------------------------------------------------------------------------ flat SGD
class Flat:
    """p, g, m on the device with a guard element after each, and the fp32 inputs on the CPU."""

    def __init__(self, n, hp, taken, cuda, seed=0):
        gen = torch.Generator().manual_seed(100 + n + seed)
        self.n, self.hp = n, hp
        self.p0 = torch.randn(n, generator=gen)
        self.g0 = torch.randn(n, generator=gen) * 0.05
        self.m0 = torch.randn(n, generator=gen) * 0.05
        if taken == 0:  # the buffer the first step must ignore
            self.m0 = torch.randn(n, generator=gen) * 1e3
            self.m0[::3] = float("nan")
        self.bufs = [torch.cat([t, torch.tensor([123.0])]).to(cuda) for t in (self.p0, self.g0, self.m0)]
        self.p, self.g, self.m = (b[:n] for b in self.bufs)

    def step(self, t, gs=1.0, counter=None, lr=oc.LR, lr_tab=None, epilogue=None):
        hp = self.hp
        sgd_flat_(self.p, self.g, self.m if hp.momentum else None, t, lr, hp.momentum, hp.dampening, hp.nesterov, hp.wd,
                  grad_scale=gs, step_counter=counter, lr_tab=lr_tab, epilogue=epilogue)

    def check(self, taken, gs=1.0):
        torch.cuda.synchronize()
        assert all(float(b[self.n]) == 123.0 for b in self.bufs)  # nothing past the end
        assert torch.equal(self.g.cpu(), self.g0)  # the gradient is not rewritten
        ref = oc.reference(self.p0, self.g0 * gs, self.m0, None, self.hp, taken)  # (gs a power of two: exact)
        got = (self.p.cpu(), self.m.cpu() if self.hp.momentum else None, None)
        assert oc.inside(got, ref), oc.excess(got, ref)
        if not self.hp.momentum:
            assert torch.equal(self.m.cpu().nan_to_num(), self.m0.nan_to_num())  # never touched


SGD_VARIANTS = [v for v in oc.VARIANTS if oc.VARIANTS[v].kind == "sgd"]


@pytest.mark.parametrize("variant", SGD_VARIANTS)
@pytest.mark.parametrize("n", [1027, 5])
def test_flat_sgd_step(n, variant, cuda):
    """The float4 loop plus the three-element tail, and a buffer shorter than two float4s: host t and the device
    counter (which already includes the step: the first is 1), grad_scale, and a rate table whose entry differs from
    the scalar rate."""
    hp = oc.VARIANTS[variant]
    for taken in oc.STEP_COUNTS:
        for gs in (1.0, 0.125):
            s = Flat(n, hp, taken, cuda)
            s.step(taken + 1, gs)  # host step count
            s.check(taken, gs)
            s = Flat(n, hp, taken, cuda)
            counter = torch.full((1,), taken + 1, dtype=torch.int32, device=cuda)
            s.step(1 if taken else 5, gs, counter=counter)  # the host count is ignored: the counter decides
            s.check(taken, gs)
            assert int(counter.item()) == taken + 1  # read, not advanced
            s = Flat(n, hp, taken, cuda)
            s.step(1, gs, counter=counter, lr=oc.LR_BASE, lr_tab=_table(taken, cuda))
            s.check(taken, gs)


def test_flat_sgd_step_epilogue_is_flat_adams(cuda):
    """loss_out[*cursor] = *loss_slot inside the cap, cursor += 1: dct_adam_flat_step's bookkeeping on the same inputs."""
    nat = native()
    hp = oc.VARIANTS["sgd_m"]
    st = torch.cuda.current_stream().cuda_stream
    for start in (2, 5):  # inside the cap of 4, and past it
        outs = []
        for which in ("sgd", "adam"):
            s = Flat(1027, hp, 3, cuda)
            cursor = torch.full((1,), start, dtype=torch.int32, device=cuda)
            slot = torch.tensor([3.5], device=cuda)
            loss_out = torch.zeros(5, device=cuda)
            counter = torch.full((1,), 4, dtype=torch.int32, device=cuda)
            if which == "sgd":
                s.step(1, counter=counter, epilogue=(cursor, slot, loss_out[:4]))
                s.check(3)
            else:
                v = torch.rand(1027, device=cuda) * 1e-3
                nat.adam_flat_step(s.p.data_ptr(), s.g.data_ptr(), s.m.data_ptr(), v.data_ptr(), 0, 1027, oc.LR, 0.9,
                                   0.999, 1e-8, 0.0, 1, 1.0, 0, counter.data_ptr(), cursor.data_ptr(), slot.data_ptr(),
                                   loss_out.data_ptr(), 4, st)
            torch.cuda.synchronize()
            outs.append((int(cursor.item()), loss_out.cpu()))
        assert outs[0][0] == outs[1][0] == start + 1 and torch.equal(outs[0][1], outs[1][1])
        assert float(outs[0][1][2]) == (3.5 if start == 2 else 0.0) and float(outs[0][1][4]) == 0.0


def test_flat_sgd_launcher_refusals(cuda):
    nat = native()
    s = Flat(1027, oc.VARIANTS["sgd_m"], 3, cuda)
    st = torch.cuda.current_stream().cuda_stream
    p, g, m = s.p.data_ptr(), s.g.data_ptr(), s.m.data_ptr()

    def raw(p=p, g=g, m=m, n=1024, mu=0.9, damp=0.0, nest=False, wd=0.0, counter=0, cursor=0, slot=0, tab=0):
        nat.sgd_flat_step(p, g, m, n, oc.LR, mu, damp, nest, wd, 1, 1.0, counter, cursor, slot, 0, 0, st, tab)

    for bad in (dict(p=p + 4), dict(g=g + 4), dict(m=m + 8), dict(mu=-0.1), dict(wd=-0.1), dict(nest=True, damp=0.1),
                dict(nest=True, mu=0.0), dict(m=0), dict(cursor=s.bufs[0].data_ptr()),
                dict(tab=_table(0, cuda).data_ptr())):  # (a table without the device counter)
        with pytest.raises(RuntimeError, match="sgd_flat_step"):
            raw(**bad)
    torch.cuda.synchronize()
    assert torch.equal(s.p.cpu(), s.p0) and torch.equal(s.m.cpu(), s.m0)  # nothing ran
    raw(mu=0.0, m=0)  # without momentum the buffer may be null
    torch.cuda.synchronize()
    assert not torch.equal(s.p.cpu(), s.p0)
    for bad in (dict(momentum=-1.0), dict(weight_decay=-1.0), dict(momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError):
            sgd_flat_(s.p, s.g, s.m, 1, oc.LR, **bad)


# ------------------------------------------------------------------------------------------------ refusals, the plan
def test_refusals_and_the_plan(cuda):
    dims, B = case = oc.CASES[1]
    d = wc.inputs(case)
    X, Y, idx = _dev(d, cuda)
    n_items = d["idx"].numel()
    p = d["p"].to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(4, device=cuda)
    tile = FusedMLPKernel(dims, bmax=1024)
    for b in (1, 4, 16, 17, 1024):
        assert tile.plan.trainer(b, optimizer="sgd") == "tile"
    assert tile.plan.trainer(1025, optimizer="sgd") == "none"
    assert native().MlpPlan([5, 300, 2], 16).trainer(4, optimizer="sgd") == "none"  # a non-tile shape

    def train(k, batch=B, **kw):
        k.train(p, m, v, X, Y, idx, n_items=n_items, batch=batch, steps=1, t0=0, lr=oc.LR, loss_out=losses, **kw)

    small = FusedMLPKernel(dims, bmax=4)
    for kind in ("sgd", "adamw"):
        with pytest.raises(ValueError, match="batch-tiled"):
            train(small, batch=4, optimizer=kind)
        with pytest.raises(ValueError, match="batch-tiled trainer's plan"):  # and the native layer on its own
            small.plan.train(p.data_ptr(), m.data_ptr(), v.data_ptr(), 0, X.data_ptr(), X.stride(0), Y.data_ptr(),
                             idx.data_ptr(), n_items, 4, 1, 0, oc.LR, 0.9, 0.999, 1e-8, 0.0, 0.0, 0, 0,
                             losses.data_ptr(), 0, 0, 0, 0, optimizer=kind)
    for bad in (dict(optimizer="rmsprop"), dict(optimizer="sgd", momentum=-0.5), dict(optimizer="sgd", weight_decay=-1.0),
                dict(optimizer="adamw", weight_decay=-1.0), dict(optimizer="sgd", nesterov=True),
                dict(optimizer="sgd", nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError):
            train(tile, **bad)
        ws = tile._tile_args(p.device, B)
        with pytest.raises(ValueError):  # the native layer refuses the same combinations
            tile.plan.train(p.data_ptr(), m.data_ptr(), v.data_ptr(), 0, X.data_ptr(), X.stride(0), Y.data_ptr(),
                            idx.data_ptr(), n_items, B, 1, 0, oc.LR, 0.9, 0.999, 1e-8, bad.get("weight_decay", 0.0), 0.0,
                            0, 0, losses.data_ptr(), 0, 0, 0, 0, optimizer=bad["optimizer"],
                            momentum=bad.get("momentum", 0.0), dampening=bad.get("dampening", 0.0),
                            nesterov=bad.get("nesterov", False), **ws)
    with pytest.raises(ValueError, match="momentum buffer"):
        k = tile
        k.train(p, None, None, X, Y, idx, n_items=n_items, batch=B, steps=1, t0=0, lr=oc.LR, optimizer="sgd", momentum=0.9)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), d["p"]) and not bool(m.any()) and not bool(v.any()) and not bool(losses.any())
    train(tile, optimizer="sgd", momentum=0.9)  # and the launch that is right does run: p and m move, v does not
    torch.cuda.synchronize()
    assert not torch.equal(p.cpu(), d["p"]) and bool(m.any()) and not bool(v.any()) and float(losses[0]) > 0


# ------------------------------------------------------------------------------------------------ Trainer.fit
class _StepLRModel(MLPClassifier):
    def configure_optimizers(self):
        opt = super().configure_optimizers()
        return {"optimizer": opt, "lr_scheduler": {"scheduler": S.StepLR(opt, step_size=2, gamma=0.5),
                                                   "interval": "step"}}


TRAINER_MODELS = {
    "sgd": (MLPClassifier, dict(optimizer="sgd", momentum=0.9, nesterov=True)),
    "adamw": (MLPClassifier, dict(optimizer="adamw", weight_decay=0.05)),
    "sgd_steplr": (_StepLRModel, dict(optimizer="sgd", momentum=0.9, nesterov=True)),
}


@pytest.mark.parametrize("B", [4, 40])
@pytest.mark.parametrize("which", list(TRAINER_MODELS))
def test_trainer_fit_on_the_fused_engine(which, B):
    """Trainer(engine="auto").fit of an SGD / AdamW model on the GPU: the fused engine on the tile plan (before this
    optimizer reached the fold: the autograd engine), and the trajectory of the CPU autograd run of the same seed, inside
    test_accum_gpu.py::test_trainer_fit_on_the_fused_engine's thresholds.  One of the runs follows a StepLR
    step-interval schedule: the rate table reaches the SGD fold."""
    cls, kw = TRAINER_MODELS[which]
    every, steps = 3, 7
    n_train, n_val = (steps - 1) * B + 3, 50

    def fit(acc):
        from dct_amd.tracking import InMemoryLogger

        seed_everything(42)
        x, y = weather_tensors(n_train + n_val, seed=0)
        tr, va = random_split(TensorPairDataset(x, y), [n_train, n_val])
        torch.manual_seed(0)
        model = cls(5, (64,), dropout=0, **kw)
        logger = InMemoryLogger()
        t = Trainer(max_epochs=1, accelerator=acc, engine="auto", logger=logger, num_sanity_val_steps=0,
                    verbose=False, log_every_n_steps=every)
        t.fit(model, DataLoader(tr, batch_size=B, shuffle=True), DataLoader(va, batch_size=B))
        return t, logger, torch.cat([q.detach().reshape(-1).cpu() for q in model.parameters()])

    t, logger, _ = fit("gpu")
    eng = t.engine
    assert eng.name == "fused" and eng.kernel.plan.use_tile and eng.step_mode == "fused-persistent"
    assert eng.kind == kw["optimizer"] and eng.kernel.plan.trainer(B, optimizer=eng.kind) == "tile"
    assert t.global_step == eng.global_step == steps == int(eng.step_counter.item())
    c, clog, want = fit("cpu")
    assert c.engine.name == "autograd" and c.global_step == steps
    err = (eng.p.cpu() - want).abs()
    print("%s B %d: param err median %.3e max %.3e, val_loss gpu %.6f cpu %.6f" % (
        which, B, err.median(), err.max(), t.callback_metrics["val_loss"], c.callback_metrics["val_loss"]))
    assert err.median() < 1e-5 and err.max() < 2e-3
    assert abs(t.callback_metrics["val_loss"] - c.callback_metrics["val_loss"]) < 5e-3
    hist, chist = logger.history("train_loss"), clog.history("train_loss")
    assert [s for s, _ in hist] == [s for s, _ in chist] == [2, 5]
    assert [v for _, v in hist] == pytest.approx([v for _, v in chist], abs=2e-4, rel=1e-3)
    if which == "sgd_steplr":
        assert eng.lr_schedule is not None and eng.lr_schedule.name == "lr-SGD"
        assert (want - torch.cat([q.detach().reshape(-1) for q in _plain_fit_params(B, n_train, n_val)])).abs().max() > 1e-4


def _plain_fit_params(B, n_train, n_val):
    """The same CPU fit without the schedule (what a fold that ignored the table would track)."""
    seed_everything(42)
    x, y = weather_tensors(n_train + n_val, seed=0)
    tr, va = random_split(TensorPairDataset(x, y), [n_train, n_val])
    torch.manual_seed(0)
    model = MLPClassifier(5, (64,), dropout=0, optimizer="sgd", momentum=0.9, nesterov=True)
    t = Trainer(max_epochs=1, accelerator="cpu", engine="auto", logger=None, num_sanity_val_steps=0, verbose=False)
    t.fit(model, DataLoader(tr, batch_size=B, shuffle=True), DataLoader(va, batch_size=B))
    return list(model.parameters())


# ------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_checkpoint_round_trip(kind):
    """One epoch, then torch's own optimizer loads the engine's state dict; a second engine resumed from it takes the
    uninterrupted run's next step bit for bit."""
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import FusedMLPEngine, optim_hparams_of

    B = 24
    kw = dict(optimizer="sgd", momentum=0.9) if kind == "sgd" else dict(optimizer="adamw", weight_decay=0.05)
    x, y = weather_tensors(400, seed=1)
    rows = torch.randperm(400, generator=torch.Generator().manual_seed(0))

    def engine():
        torch.manual_seed(0)
        model = MLPClassifier(5, hidden=(64,), dropout=0.1, **kw)
        ctx = init_distributed("gpu")
        eng = FusedMLPEngine(model, ctx, B, seed=42, adam=optim_hparams_of(model.configure_optimizers()))
        eng.attach_data(x, y, rows[:340], rows[340:])
        return model, eng

    model, eng = engine()
    assert eng.optimizer_state_dict()["state"] == {}  # no step taken: torch has no state either
    eng.train_epoch(0)
    steps = math.ceil(340 / B)
    assert eng.global_step == steps == int(eng.step_counter.item())
    sd = eng.optimizer_state_dict()
    opt = model.configure_optimizers()  # a fresh torch optimizer of the model's own kind
    opt.load_state_dict(sd)
    shapes = [q.shape for q in model.parameters()]
    key = "momentum_buffer" if kind == "sgd" else "exp_avg"
    off = 0
    for q, shape in zip(model.parameters(), shapes):
        n = shape.numel()
        assert torch.equal(opt.state[q][key].cpu(), eng.m[off:off + n].view(shape).cpu())
        if kind == "adamw":
            assert torch.equal(opt.state[q]["exp_avg_sq"].cpu(), eng.v[off:off + n].view(shape).cpu())
            assert float(opt.state[q]["step"]) == eng.global_step
        else:
            assert set(opt.state[q]) == {"momentum_buffer"}
        off += n
    assert set(sd["param_groups"][0]) == set(model.configure_optimizers().state_dict()["param_groups"][0])
    _, resumed = engine()
    resumed.p.copy_(eng.p)
    resumed.load_optimizer_state(sd, eng.global_step)
    assert int(resumed.step_counter.item()) == steps and torch.equal(resumed.m, eng.m)
    outs = []
    for e in (eng, resumed):
        n = e.upload_epoch_indices(1)
        loss = torch.zeros(4, device=e.device)
        e.run_steps(n, 1, loss, first_step=0)
        torch.cuda.synchronize()
        outs.append((e.p.cpu(), e.m.cpu(), e.v.cpu(), loss.cpu()))
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(outs[0][0], model_flat(model))  # (the step moved the parameters)


def model_flat(model):
    return torch.cat([q.detach().reshape(-1).cpu() for q in model.parameters()])


# ------------------------------------------------------------------------------------------------ DDP step path
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("graph", ["1", "0"])
def test_ddp_step_path_world1_matches_persistent(graph, kind, monkeypatch):
    """DCT_FORCE_DDP=1 at world size 1 (grad-mode launch -> one-rank all-reduce -> flat SGD / flat Adam with decoupled
    decay, HIP-graph chunks of 7) reproduces the train-mode launches over 39 steps; the tolerances of
    test_accum_gpu.py::test_accumulating_ddp_step_path_world1_matches_persistent."""
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import FusedMLPEngine, optim_hparams_of

    kw = dict(optimizer="sgd", momentum=0.9) if kind == "sgd" else dict(optimizer="adamw", weight_decay=0.05)
    B, steps = 24, 39
    x, y = weather_tensors(1200, seed=1)
    rows = torch.randperm(1200, generator=torch.Generator().manual_seed(0))
    n_train = (steps - 1) * B + 16

    def run(force):
        monkeypatch.setenv("DCT_FORCE_DDP", force)
        monkeypatch.setenv("DCT_GRAPH", graph)
        monkeypatch.setattr(FusedMLPEngine, "GRAPH_CHUNK", 7)
        torch.manual_seed(0)
        model = MLPClassifier(5, hidden=(64,), dropout=0.0, **kw)
        ctx = init_distributed("gpu")
        eng = FusedMLPEngine(model, ctx, B, seed=42, adam=optim_hparams_of(model.configure_optimizers()))
        assert eng.kernel.plan.use_tile and not eng.fused_update and eng.xg is None and eng.gx is None
        eng.attach_data(x, y, rows[:n_train], rows[n_train:])
        assert eng.steps_per_epoch() == steps
        n = eng.upload_epoch_indices(0)
        loss = torch.zeros(64, device=ctx.device)
        eng.run_steps(n, 20, loss, first_step=0)
        eng.run_steps(n, 19, loss, first_step=20)
        torch.cuda.synchronize()
        assert int(eng.step_counter.item()) == steps
        return eng.p.cpu(), eng.m.cpu(), loss[:steps].cpu(), eng

    p0, m0, l0, e0 = run("0")
    p1, m1, l1, e1 = run("1")
    assert e0.step_mode == "fused-persistent" and e1.ddp and e1.comm is not None
    assert e1.graph_used == (graph == "1")
    assert torch.allclose(l0, l1, atol=1e-4), (l0 - l1).abs().max()
    assert (p0 - p1).abs().max() < 1e-3 and (p0 - p1).abs().median() < 1e-5
    assert torch.allclose(m0, m1, atol=1e-4) and bool(m0.any())


def test_required_xgmi_exchange_with_a_non_adam_model_raises(monkeypatch, cuda):
    """DCT_ALLREDUCE=xgmi: the tile plan has no in-kernel exchange and the peer all-reduce kernel applies Adam, so a
    distributed SGD / AdamW engine has neither - the existing error, before any peer buffer is set up.  (A stand-in
    two-rank context on the control plane that shares a device: no second process, no collective.)"""
    import types

    from dct_amd.trainer.engines import FusedMLPEngine, optim_hparams_of

    monkeypatch.setenv("DCT_ALLREDUCE", "xgmi")
    ctx = types.SimpleNamespace(device=cuda, rank=0, world_size=2, is_distributed=True, backend="gloo",
                                broadcast_=lambda t, src=0: t)
    for kw in (dict(optimizer="sgd", momentum=0.9), dict(optimizer="adamw", weight_decay=0.05)):
        torch.manual_seed(0)
        model = MLPClassifier(5, hidden=(64,), dropout=0.0, **kw)
        with pytest.raises(RuntimeError, match="neither the in-kernel exchange nor the peer"):
            FusedMLPEngine(model, ctx, 4, seed=42, adam=optim_hparams_of(model.configure_optimizers()))
