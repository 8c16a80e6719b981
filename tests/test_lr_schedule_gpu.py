"""The device learning-rate table on the GPU (csrc/lr_table.h): every flat-Adam launch form reading its rate from the
table, a captured step following the table across replays, the wide-MLP step executor, and Trainer.fit with a scheduler
(tests/lr_cases.py).

Flat Adam: each launch with the table is compared (a) bit for bit with the same launch given the table's entry as its
scalar rate and no table, and (b) with adam_one in fp64 at that rate under the bounds tests/wide_step_cases.py counts
for p, m and v (tests/clip_cases.py's for the clipped forms).  Every table launch is also handed a scalar rate far
from the table's (lr_cases.SCALAR_LR): a launch that ignores its table lands outside the bounds."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch.optim import lr_scheduler as S
from torch.utils.data import DataLoader

import clip_cases as K
import dct_amd  # noqa: F401
import lr_cases as L
import wide_step_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _collect_engines_outside_a_capture():
    """A Trainer and its module refer to each other, so a fit's engine - captured graphs, the executor's buffers, the
    rate table - is released by the garbage collector.  Collect at the end of each test, where no capture is open."""
    yield
    import gc

    torch.cuda.synchronize()
    gc.collect()


def _nat():
    from dct_amd.ops._native import native

    return native()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ratio(what, got, want, bound):
    got = got.double().cpu()
    if not bool(torch.isfinite(got).all()):
        print("  %s: non-finite values" % what)
        return float("inf")
    r = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
    print("  %s: worst error / bound %.4f" % (what, r))
    return r


def _table(img=None):
    """The window of lr_cases on the device, a guard word after it."""
    img = L.window_image() if img is None else img
    return torch.cat([img, torch.tensor([0x7FC00000], dtype=torch.int32)]).to(_dev()).view(torch.float32)


class State:
    """p, g, m, v on the device, a guard element after each; launches through every flat-Adam form."""

    def __init__(self, n, scale="unit", seed=0):
        self.n = n
        self.cpu = C.adam_inputs(n, scale, seed)
        self.init = [torch.cat([x, torch.full((1,), 123.0)]).to(_dev()) for x in self.cpu]
        self.reset()

    def reset(self):
        self.p, self.g, self.m, self.v = (x.clone() for x in self.init)

    def out(self):
        return tuple(x.clone() for x in (self.p, self.m, self.v))

    def launch(self, form, hp, counter, lr_tab, clip=None, parts=((), (), (), ()), lo=0, hi=None):
        nat, n = _nat(), self.n
        ptrs = (self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), 0)
        tab = 0 if lr_tab is None else lr_tab.data_ptr()
        hyp = (hp.lr, hp.b1, hp.b2, hp.eps, hp.wd)
        sc = counter.data_ptr()
        if form == "adam_flat":
            nat.adam_flat(*ptrs, n, *hyp, 1, hp.grad_scale, hp.decoupled, sc, _st(), tab)
        elif form == "adam_flat_step":
            nat.adam_flat_step(*ptrs, n, *hyp, 1, hp.grad_scale, hp.decoupled, sc, 0, 0, 0, 0, _st(), tab)
        elif form == "clipped":
            coef, value = clip
            nat.adam_flat_step_clipped(*ptrs, n, *hyp, 1, hp.grad_scale, hp.decoupled, sc, 0, 0, 0, 0,
                                       0 if coef is None else coef.data_ptr(), value, _st(), tab)
        elif form == "parts":
            nat.adam_flat_step_parts(*ptrs, n, *hyp, hp.grad_scale, hp.decoupled, sc, 0, 0, 0, 0, *parts, _st(), tab)
        elif form == "adam_range":
            r = nat.AdamRange(*ptrs, n, *hyp, hp.grad_scale, hp.decoupled, sc, *parts, lo, n if hi is None else hi, tab)
            nat.adam_range(r, 0, 0, 0, 0, _st())
        else:
            raise AssertionError(form)
        torch.cuda.synchronize()
        for x in (self.p, self.m, self.v):
            assert float(x[n]) == 123.0, form + ": wrote past n"
        assert torch.equal(_bits(self.g), _bits(self.init[1])), form + ": g changed"

    def check(self, what, ref):
        n = self.n
        rp = _ratio(what + " p", self.p[:n], ref.p, ref.p_bound)
        rm = _ratio(what + " m", self.m[:n], ref.m, ref.m_bound)
        rv = _ratio(what + " v", self.v[:n], ref.v, ref.v_bound)
        assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0, (what, rp, rm, rv)


def _counter(taken):
    """The device step count an Adam launch sees: it already includes the step being applied."""
    return torch.tensor([taken + 1], dtype=torch.int32, device=_dev())


def _table_vs_scalar(s, form, base, ref_of, **kw):
    """For every edge of lr_cases.TAKEN: the table launch (scalar rate SCALAR_LR, ignored) == the scalar launch at the
    table's entry, bit for bit, and both inside the fp64 bounds at that rate.  Returns the distinct p results."""
    tab = _table()
    seen = set()
    for taken, why in L.TAKEN.items():
        hp = L.hyper_at(base, taken)
        s.reset()
        s.launch(form, base._replace(lr=L.SCALAR_LR), _counter(taken), tab, **kw)
        with_tab = s.out()
        s.check("%s table, %d taken (%s)" % (form, taken, why), ref_of(hp, taken + 1))
        s.reset()
        s.launch(form, hp, _counter(taken), None, **kw)
        for a, b, name in zip(with_tab, s.out(), "pmv"):
            assert torch.equal(_bits(a), _bits(b)), "%s %d taken: %s differs from the scalar launch" % (form, taken, name)
        seen.add(hp.lr)
    assert len(seen) == 3  # first entry (twice: clamped from below, and itself), peak, last entry (itself, clamped)
    assert float(tab[-1]) != float(tab[-1])  # the guard word after the table is still the NaN it was


# ---------------------------------------------------------------------------------------------- (a) flat Adam forms
@pytest.mark.parametrize("hyper", list(L.ADAM_HYPERS))
@pytest.mark.parametrize("form", ["adam_flat", "adam_flat_step", "adam_range"])
def test_flat_adam_reads_its_rate_from_the_table(form, hyper):
    """n = 1027: the float4 loop and the three-element tail.  AdamW: the decoupled decay term lr * wd * p too."""
    s = State(L.ADAM_N_TAIL, seed=11)
    base = L.ADAM_HYPERS[hyper]
    _table_vs_scalar(s, form, base, lambda hp, t: C.adam_ref(*s.cpu, t, hp, device_counter=True))


def test_flat_adam_table_and_a_second_grid_stride_pass():
    n = L.ADAM_N_TWO_PASSES
    s = State(n, scale="tabular", seed=1)
    tab, taken = _table(), 5
    base = L.ADAM_HYPERS["adamw"]
    hp = L.hyper_at(base, taken)
    ref = C.adam_ref(*s.cpu, taken + 1, hp, device_counter=True)
    for form in ("adam_flat", "adam_range"):
        s.reset()
        s.launch(form, base._replace(lr=L.SCALAR_LR), _counter(taken), tab)
        with_tab = s.out()
        s.check("%s n = %d" % (form, n), ref)
        s.reset()
        s.launch(form, hp, _counter(taken), None)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(with_tab, s.out()))


@pytest.mark.parametrize("kind", ["coef", "clamp"])
def test_clipped_adam_reads_its_rate_from_the_table(kind):
    s = State(L.ADAM_N_TAIL, seed=12)
    base = L.ADAM_HYPERS["adam_scaled_l2"]
    p, g, m, v = s.cpu
    if kind == "coef":
        max_norm = K.max_norms(g, base.grad_scale)["active"]
        cref = K.clip_ref(g, base.grad_scale, max_norm)
        coef = torch.tensor([cref.coef], dtype=torch.float32, device=_dev())
        # the coefficient is handed over as an fp32 value: the reference takes that value, with no error of its own
        exact = cref._replace(coef=float(coef.item()), eps_c=0.0)
        _table_vs_scalar(s, "clipped", base, lambda hp, t: K.clipped_adam_ref(p, g, m, v, t, hp, exact,
                                                                               device_counter=True), clip=(coef, 0.0))
    else:
        c = K.value_clip(g, base.grad_scale)
        _table_vs_scalar(s, "clipped", base, lambda hp, t: K.value_adam_ref(p, g, m, v, t, hp, c, device_counter=True),
                         clip=(None, c))


@pytest.mark.parametrize("form", ["parts", "adam_range"])
def test_adam_over_split_k_partials_reads_its_rate_from_the_table(form):
    name, n, ranges, _ = C.PARTS_CASES[0]  # 1, 4 and 8 slices: the S = 8 kernel
    s = State(n, scale="tabular", seed=13)
    slices = C.part_slices(ranges, "tabular", seed=14)
    dsl = [x.to(_dev()) for x in slices]
    parts = ([r[0] for r in ranges], [r[1] for r in ranges], [x.data_ptr() for x in dsl], [r[2] for r in ranges])
    ref_parts = [(off, cnt, sp, sl) for (off, cnt, sp), sl in zip(ranges, slices)]
    base = L.ADAM_HYPERS["adamw"]
    _table_vs_scalar(s, form, base, lambda hp, t: C.adam_ref(*s.cpu, t, hp, parts=ref_parts, device_counter=True),
                     parts=parts)


def test_adam_riding_in_a_dw_launch_reads_its_rate_from_the_table():
    """The Adam range in extra workgroups of the split-K dW launch (gemm2_dw_adam_kernel, the one-element-per-thread
    body): the same table read."""
    nat = _nat()
    M, N, Kk, splits = C.DW_CASES[0][:4]
    gen = torch.Generator().manual_seed(3)
    dz = torch.randn(Kk, M, generator=gen).to(_dev(), torch.bfloat16)
    x = torch.randn(Kk, N, generator=gen).to(_dev(), torch.bfloat16)
    part = torch.zeros(splits * M * N, device=_dev())
    colsum = torch.zeros(M, device=_dev())
    s = State(L.ADAM_N_TAIL, scale="tabular", seed=15)
    base, tab = L.ADAM_HYPERS["adamw"], _table()
    for taken in (0, 5, 20):
        hp = L.hyper_at(base, taken)
        res = []
        for h, t in ((base._replace(lr=L.SCALAR_LR), tab.data_ptr()), (hp, 0)):
            s.reset()
            r = nat.AdamRange(s.p.data_ptr(), s.g.data_ptr(), s.m.data_ptr(), s.v.data_ptr(), 0, s.n, h.lr, h.b1, h.b2,
                              h.eps, h.wd, h.grad_scale, h.decoupled, _counter(taken).data_ptr(), [], [], [], [], 0,
                              s.n, t)
            nat.gemm_bf16_dw_partials_adam(dz.data_ptr(), x.data_ptr(), part.data_ptr(), colsum.data_ptr(), M, N, Kk,
                                           splits, r, 0, _st())
            torch.cuda.synchronize()
            res.append(s.out())
        s.check("riding Adam, %d taken" % taken, C.adam_ref(*s.cpu, taken + 1, hp, device_counter=True))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*res))


def test_table_launches_refuse_what_they_cannot_read():
    s = State(64, seed=16)
    tab = _table()
    hp = L.ADAM_HYPERS["adam"]._replace(lr=1e-3)
    nat = _nat()
    ptrs = (s.p.data_ptr(), s.g.data_ptr(), s.m.data_ptr(), s.v.data_ptr(), 0)
    hyp = (hp.lr, hp.b1, hp.b2, hp.eps, hp.wd)
    with pytest.raises(RuntimeError):  # a table without a device step count to index it
        nat.adam_flat(*ptrs, 64, *hyp, 1, 1.0, 0, 0, _st(), tab.data_ptr())
    with pytest.raises(RuntimeError):  # a header that is not one aligned word
        nat.adam_flat(*ptrs, 64, *hyp, 1, 1.0, 0, _counter(0).data_ptr(), _st(), tab.data_ptr() + 4)
    with pytest.raises(RuntimeError):
        r = nat.AdamRange(*ptrs, 64, *hyp, 1.0, 0, _counter(0).data_ptr(), [], [], [], [], 0, 64, tab.data_ptr() + 4)
        nat.adam_range(r, 0, 0, 0, 0, _st())
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((s.p, s.m, s.v), (s.init[0], s.init[2], s.init[3])))


# ---------------------------------------------------------------------------------------------- (b) captured replay
def _flat_adam(n, schedule):
    from dct_amd.ops.optim import FlatAdam

    p, g, m, v = (x.to(_dev()) for x in C.adam_inputs(n, "unit", seed=21))
    fa = FlatAdam(p.clone(), g, [p.shape], lr=L.SCALAR_LR if schedule else 1e-3, lr_schedule=schedule)
    fa.m.copy_(m)
    fa.v.copy_(v)
    return fa


def _window_schedule(t0=L.WINDOW_T0, rates=L.WINDOW):
    """An LrSchedule whose device table holds the given window."""
    from dct_amd.trainer.lr_schedule import LrSchedule

    opt = L.new_optimizer()
    sched = LrSchedule(opt, S.LambdaLR(opt, lambda k: 1.0), "step")
    sched.set_window(t0, rates, device=_dev())
    return sched


def test_captured_flat_adam_step_follows_the_table_across_replays():
    """The rate is read from the table at the device step count, not baked into the graph: one captured step, replayed 5
    times over a varying window (3 steps taken before: the window's first entry, then on to its peak and down), each
    replay equal, bit for bit, to an eager step of a second optimizer given that step's rate as its scalar."""
    n, first = 1027, L.WINDOW_T0
    fa = _flat_adam(n, _window_schedule())
    eager = _flat_adam(n, None)
    for x in (fa, eager):
        x.step_count = first
        x.sync_device_counter()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(_dev())
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            fa.step()
    torch.cuda.current_stream().wait_stream(s)
    fa.step_count -= 1  # capture recorded without executing
    fa._device_counter().fill_(first)
    rates = set()
    for k in range(5):
        g.replay()
        fa.step_count += 1
        rate = L.table_rate(L.window_image(), first + k)
        rates.add(rate)
        eager.param_groups[0]["lr"] = rate
        eager.step()
        torch.cuda.synchronize()
        for a, b, name in ((fa.p, eager.p, "p"), (fa.m, eager.m, "m"), (fa.v, eager.v, "v")):
            assert torch.equal(_bits(a), _bits(b)), "replay %d: %s differs from the eager step at rate %g" % (k, name, rate)
    assert len(rates) == 5 and int(fa._device_counter().item()) == first + 5


# ---------------------------------------------------------------------------------------------- (c) GraphMLPEngine
G_DIMS, G_B, G_EXTRA = [64, 256, 256, 2], 1024, 300  # 5 full batches and a partial one: 6 steps
G_T0, G_RATES = 2, [5e-4, 4e-3, 1e-3]                 # rates of the 6 steps: a a a b c c (both ends clamp)
G_BASE = 2e-3


def _graph_data():
    gen = torch.Generator().manual_seed(0)
    X = torch.randn(5 * G_B + G_EXTRA, G_DIMS[0], generator=gen)
    Y = ((X @ torch.randn(G_DIMS[0], generator=gen)) > 0).long()
    return X, Y


def _graph_run(monkeypatch, dw_into_adam, scheduled):
    from dct_amd.models.mlp import MLPClassifier
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import adam_hparams_from
    from dct_amd.trainer.graph_engine import GraphMLPEngine

    monkeypatch.setenv("DCT_DW_INTO_ADAM", dw_into_adam)
    torch.manual_seed(0)
    model = MLPClassifier(G_DIMS[0], hidden=tuple(G_DIMS[1:-1]), num_classes=G_DIMS[-1], dropout=0.0, loss="ce",
                          lr=G_BASE)
    sched = _window_schedule(G_T0, G_RATES) if scheduled else None
    eng = GraphMLPEngine(model, init_distributed("gpu"), G_B, seed=42,
                         adam=adam_hparams_from(model.configure_optimizers()), use_graph=False, lr_schedule=sched)
    X, Y = _graph_data()
    rows = torch.arange(X.shape[0])
    eng.attach_data(X, Y, rows, rows[:G_B])
    losses = eng.train_epoch(0, shuffle=False).cpu()
    torch.cuda.synchronize()
    assert losses.numel() == 6 and int(eng.step_counter.item()) == 6
    return eng, losses, eng.p.cpu()


def _graph_torch_loop(rates):
    """torch.optim.Adam + a scheduler holding the window's rates, fp32, on the bf16-rounded inputs."""
    from dct_amd.models.mlp import MLPClassifier

    torch.manual_seed(0)
    model = MLPClassifier(G_DIMS[0], hidden=tuple(G_DIMS[1:-1]), num_classes=G_DIMS[-1], dropout=0.0, loss="ce", lr=G_BASE)
    opt = torch.optim.Adam(model.parameters(), lr=G_BASE)
    sched = S.LambdaLR(opt, lambda k: rates[min(k, len(rates) - 1)] / G_BASE)
    X, Y = _graph_data()
    X = X.to(torch.bfloat16).float()
    for b in range(6):
        opt.zero_grad()
        F.cross_entropy(model(X[b * G_B:(b + 1) * G_B]), Y[b * G_B:(b + 1) * G_B]).backward()
        opt.step()
        sched.step()
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def test_graph_engine_follows_the_table(monkeypatch):
    """6 steps of the wide-MLP executor over a varying window: Adam riding in the dW launches, the adam_range launch
    behind them and (partial last batch, DCT_DW_INTO_ADAM=0) the flat launches all read the table.  Against its own
    run under DCT_DW_INTO_ADAM=0 with the same table, and against torch.optim.Adam + a scheduler with the same rates,
    at the tolerances tests/test_graph_engine_gpu.py compares its constant-rate trajectories with (losses 1e-3
    absolute, parameters 1e-2 in relative norm); the constant-rate run and torch loop are further away than that."""
    e1, l1, p1 = _graph_run(monkeypatch, "1", True)
    assert e1.exe.partial_layers >= 1 and e1.exe.part_fallbacks >= 1  # (the partial last batch: the flat launches)
    e0, l0, p0 = _graph_run(monkeypatch, "0", True)
    assert e0.exe.partial_layers == 0
    step_rates = [L.table_rate(L.table_image(G_T0, G_RATES), k) for k in range(6)]
    assert len(set(step_rates)) == 3
    want = _graph_torch_loop(step_rates)
    plain = _graph_torch_loop([G_BASE] * 6)
    _, lc, pc = _graph_run(monkeypatch, "1", False)
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    print("  riding vs DCT_DW_INTO_ADAM=0: losses %.3e, parameters %.3e" % (float((l1 - l0).abs().max()), rel(p1, p0)))
    print("  vs torch + scheduler: riding %.3e, DCT_DW_INTO_ADAM=0 %.3e" % (rel(p1, want), rel(p0, want)))
    print("  power: scheduled vs constant-rate engine %.3e, scheduled vs constant-rate torch %.3e"
          % (rel(p1, pc), rel(p1, plain)))
    assert torch.isfinite(l1).all() and torch.allclose(l1, l0, atol=1e-3)
    assert rel(p1, p0) < 1e-2
    assert rel(p1, want) < 1e-2 and rel(p0, want) < 1e-2
    assert rel(p1, pc) > 3e-2 and rel(p1, plain) > 3e-2


# ---------------------------------------------------------------------------------------------- (d) Trainer.fit
def _fit_data(n, d):
    gen = torch.Generator().manual_seed(4)
    X = torch.randn(n, d, generator=gen)
    Y = ((X[:, 0] - X[:, 1]) > 0).long()
    return X, Y


def _scheduled_model(dims, kind, lr):
    from dct_amd.models.mlp import MLPClassifier

    class M(MLPClassifier):
        def configure_optimizers(self):
            opt = torch.optim.Adam(self.parameters(), lr=lr)
            if kind == "epoch":
                return {"optimizer": opt, "lr_scheduler": S.StepLR(opt, step_size=1, gamma=0.25)}
            if kind == "step":
                sched = S.LinearLR(opt, start_factor=0.1, total_iters=12)
                return {"optimizer": opt, "lr_scheduler": {"scheduler": sched, "interval": "step"}}
            return opt

    torch.manual_seed(0)
    return M(dims[0], hidden=tuple(dims[1:-1]), num_classes=dims[-1], dropout=0.0, lr=lr)


def _torch_fit(dims, kind, lr, X, Y, B, epochs):
    model = _scheduled_model(dims, kind, lr)
    from dct_amd.trainer.lr_schedule import parse_configure_optimizers

    opt, cfg = parse_configure_optimizers(model.configure_optimizers())
    steps = math.ceil(X.shape[0] / B)
    for _ in range(epochs):
        for b in range(steps):
            opt.zero_grad()
            F.cross_entropy(model(X[b * B:(b + 1) * B]), Y[b * B:(b + 1) * B]).backward()
            opt.step()
            if cfg and cfg["interval"] == "step":
                cfg["scheduler"].step()
        if cfg and cfg["interval"] == "epoch":
            cfg["scheduler"].step()
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


@pytest.mark.parametrize("kind", ["epoch", "step"])
@pytest.mark.parametrize("graph", ["1", "0"])
def test_trainer_fit_autograd_engine_on_the_gpu_follows_the_scheduler(kind, graph, monkeypatch):
    """The 5-64-2 model on the autograd engine, 2 short epochs, eager (DCT_GRAPH=0) and with the step captured after
    its warm-up steps and replayed: against the torch loop with the same data order, optimizer and scheduler (fp32 on
    both sides: max |dp| < 1e-4, the bound this suite compares a trained parameter vector with a torch.optim.Adam loop
    under, tests/test_grad_clip_cpu.py), and further than 100 times that from the fit without the scheduler."""
    from dct_amd.data.dataset import TensorPairDataset
    from dct_amd.trainer import Trainer

    monkeypatch.setenv("DCT_GRAPH", graph)
    dims, B, lr, epochs = [5, 64, 2], 4, 0.01, 2
    X, Y = _fit_data(40, 5)

    def fit(k):
        model = _scheduled_model(dims, k, lr)
        t = Trainer(max_epochs=epochs, accelerator="gpu", engine="autograd", num_sanity_val_steps=0, verbose=False)
        t.fit(model, DataLoader(TensorPairDataset(X, Y), batch_size=B, shuffle=False),
              DataLoader(TensorPairDataset(X[:B], Y[:B]), batch_size=B))
        assert t.engine.name == "autograd" and t.engine.graph_used == (graph == "1")
        return torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters()])

    got, want = fit(kind), _torch_fit(dims, kind, lr, X, Y, B, epochs)
    err = float((got - want).abs().max())
    gap = float((got - fit("none")).abs().max())
    print("  autograd engine (%s, DCT_GRAPH=%s) vs the torch loop: max |dp| = %.3e; vs no scheduler %.3e"
          % (kind, graph, err, gap))
    assert err < 1e-4 and gap > 1e-2


def test_trainer_fit_graph_engine_follows_the_scheduler_and_saves_it(tmp_path):
    """Trainer.fit on the graph engine with a step-interval scheduler: the engine stays "graph", the table holds the
    epoch's rates, and the checkpoint carries the scheduler."""
    from torch.utils.data import TensorDataset

    from dct_amd.ckpt import LearningRateMonitor, ModelCheckpoint, load_checkpoint
    from dct_amd.tracking import InMemoryLogger
    from dct_amd.trainer import Trainer

    X, Y = _fit_data(1024, 64)
    model = _scheduled_model([64, 128, 128, 2], "step", 1e-3)
    ck = ModelCheckpoint(dirpath=str(tmp_path), save_top_k=0, save_last=True)
    logger = InMemoryLogger()
    tr = Trainer(max_epochs=2, accelerator="gpu", engine="graph", verbose=False, num_sanity_val_steps=0, logger=logger,
                 callbacks=[ck, LearningRateMonitor("step")], log_every_n_steps=2)
    tr.fit(model, DataLoader(TensorDataset(X, Y), batch_size=256), DataLoader(TensorDataset(X[:256], Y[:256]), batch_size=256))
    assert tr.engine.name == "graph" and tr.global_step == 8
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    sched = S.LinearLR(opt, start_factor=0.1, total_iters=12)
    rates = []
    for _ in range(8):
        rates.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert tr.lr_schedule.t0 == 4 and tr.lr_schedule.host == rates[4:]
    img = tr.lr_schedule.table.view(torch.int32)[:8].cpu()
    assert torch.equal(img, L.table_image(4, rates[4:]))
    assert logger.history("lr-Adam") == [(k, rates[k]) for k in (1, 3, 5, 7)]
    ckpt = load_checkpoint(str(tmp_path / "last.ckpt"))
    assert ckpt["lr_schedulers"][0]["last_epoch"] == 8
    assert ckpt["optimizer_states"][0]["param_groups"][0]["lr"] == pytest.approx(sched.get_last_lr()[0], rel=1e-12)


# ---------------------------------------------------------------------------------------------- (e) persistent trainers
def _family_launches(monkeypatch, name, launches):
    """launches [(first step, steps, t0, lr, table or None)] of a family of lr_cases.FAMILIES from the same start;
    (p, m, v, losses) on the CPU."""
    import block5_sched_cases as bc
    from dct_amd.ops.fused_mlp import FusedMLPKernel

    env, dims, B, bmax, steps, short, trainer, single = L.FAMILIES[name]
    for k_, v_ in env.items():
        monkeypatch.delenv(k_, raising=False) if v_ is None else monkeypatch.setenv(k_, v_)
    _nat().reload_knobs()
    n_items = steps * B - short
    X, Y, idx, p0 = bc.sized_data(dims, n_items, 17, 5)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    losses = torch.zeros(steps, device=_dev())
    k = FusedMLPKernel(dims, bmax=bmax)
    prof = torch.zeros(64, dtype=torch.int64, device=_dev()) if single else None
    assert k.plan.trainer(B, mode=0, steps=steps, prof=single) == trainer
    assert sum(n for _, n, _, _, _ in launches) == steps
    for first, n, t0, lr, tab in launches:
        k.train(p, m, v, X, Y, idx[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=t0, lr=lr,
                weight_decay=0.01, dropout=0.0, seed=3, step_base=t0, loss="ce",
                loss_out=losses[first:], prof=prof, lr_tab=tab)
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu(), losses.cpu()


def _family_fp64(name, step_rates):
    """torch.optim.Adam (coupled weight decay 0.01) in fp64 over the family's batches, step k at step_rates[k], the
    step count starting at FAMILY_START: (p, m, v, losses)."""
    import block5_sched_cases as bc

    _, dims, B, _, steps, short, _, _ = L.FAMILIES[name]
    n_items = steps * B - short
    X, Y, idx, p0 = (t.cpu() for t in bc.sized_data(dims, n_items, 17, 5))
    layers, off = [], 0
    for i in range(len(dims) - 1):
        lin = torch.nn.Linear(dims[i], dims[i + 1]).double()
        with torch.no_grad():
            lin.weight.copy_(p0[off: off + lin.weight.numel()].view_as(lin.weight))
            off += lin.weight.numel()
            lin.bias.copy_(p0[off: off + lin.bias.numel()])
            off += lin.bias.numel()
        layers += [lin] + ([torch.nn.ReLU()] if i < len(dims) - 2 else [])
    net = torch.nn.Sequential(*layers)
    params = list(net.parameters())
    opt = torch.optim.Adam(params, lr=1.0, weight_decay=0.01)
    for q in params:
        opt.state[q] = dict(step=torch.tensor(float(L.FAMILY_START)), exp_avg=torch.zeros_like(q),
                            exp_avg_sq=torch.zeros_like(q))
    losses = []
    for k in range(steps):
        rows = idx[k * B:(k + 1) * B].long()
        opt.param_groups[0]["lr"] = step_rates[k]
        opt.zero_grad()
        loss = F.cross_entropy(net(X[rows].double()), Y[rows].long())
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])  # noqa: E731
    return (flat(params), flat([opt.state[q]["exp_avg"] for q in params]),
            flat([opt.state[q]["exp_avg_sq"] for q in params]), torch.tensor(losses, dtype=torch.float64))


def _inside_trajectory_bounds(what, got, ref):
    """The project's trajectory bounds (tests/test_mlp_tile_gpu._check_against_torch, which tests/test_lds_trainer_gpu
    and tests/test_dropout_reference_gpu hold these kernels to): parameter error median < 1e-5 and max < 2e-3, losses
    atol 2e-4 rtol 1e-3, m and v atol 1e-4 rtol 1e-2.  Prints each figure, returns whether all hold."""
    p, m, v, losses = (t.double() for t in got)
    err = (p - ref[0]).abs()
    figs = dict(p_median=float(err.median()), p_max=float(err.max()), loss=float((losses - ref[3]).abs().max()),
                m=float((m - ref[1]).abs().max()), v=float((v - ref[2]).abs().max()))
    print("  %s vs fp64: %s" % (what, ", ".join("%s %.3e" % kv for kv in figs.items())))
    return (figs["p_median"] < 1e-5 and figs["p_max"] < 2e-3
            and torch.allclose(losses, ref[3], atol=2e-4, rtol=1e-3)
            and torch.allclose(m, ref[1], atol=1e-4, rtol=1e-2) and torch.allclose(v, ref[2], atol=1e-4, rtol=1e-2))


def _equal(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _same(what, a, b):
    for name, x, y in zip("pmvl", a, b):
        assert torch.isfinite(x).all(), (what, name)
        assert torch.equal(_bits(x), _bits(y)), (what, name, float((x - y).abs().max()))
    assert bool((a[3] != 0).all())


@pytest.mark.parametrize("name", list(L.FAMILIES))
def test_persistent_trainer_reads_its_rate_from_the_table(name, monkeypatch):
    """(a) a table whose entries all equal lr reproduces the scalar launch bit for bit (p, m, v, losses); (b) one
    K-step launch over a varying window (warm-up then decay, t0 != 0, steps below and past it: both clamps) equals K
    one-step launches of the same kernel, each given the table's entry as its scalar, t0 and the dropout step advanced
    as the two-launch tests of tests/block5_sched_cases.py do; (c) the premise: (b) at a constant rate with no table.

    Where (c) does not hold - a kernel that keeps its Adam moments in another form in registers than in memory rounds
    them once more at every launch boundary, so its K one-step launches are not its K-step launch even at a constant
    rate: existing behaviour - (b) is compared instead with torch.optim.Adam in fp64 at the table's per-step rates
    under the project's trajectory bounds (_inside_trajectory_bounds), and so are the K one-step launches; the
    constant-rate launch must land outside those bounds of the scheduled reference."""
    steps = L.FAMILIES[name][4]
    S0, lr = L.FAMILY_START, L.FAMILY_LR
    t0w, rates = L.family_window(steps)
    img = L.table_image(t0w, rates)
    step_rates = [L.f32(L.table_rate(img, S0 + k)) for k in range(steps)]
    assert step_rates[0] == step_rates[2] != step_rates[3] and step_rates[-1] == step_rates[-3] != step_rates[-4]
    whole = lambda rate, tab: [(0, steps, S0, rate, tab)]  # noqa: E731
    single = lambda rs: [(k, 1, S0 + k, rs[k], None) for k in range(steps)]  # noqa: E731
    scalar = _family_launches(monkeypatch, name, whole(lr, None))
    _same("(a) constant table", _family_launches(monkeypatch, name, whole(0.5, _table(L.table_image(t0w, [lr] * len(rates))))),
          scalar)
    premise = _equal(scalar, _family_launches(monkeypatch, name, single([lr] * steps)))
    varying = _family_launches(monkeypatch, name, whole(0.5, _table(img)))
    stepwise = _family_launches(monkeypatch, name, single(step_rates))
    assert not torch.equal(varying[0], scalar[0])
    print("  %s: premise (c) %s" % (name, "holds" if premise else "does not hold: (b) against fp64"))
    if premise:
        _same("(b) varying table", varying, stepwise)
        return
    ref = _family_fp64(name, step_rates)
    assert _inside_trajectory_bounds("(b) K-step launch with the table", varying, ref)
    assert _inside_trajectory_bounds("(b) K one-step launches at the table's rates", stepwise, ref)
    assert not _inside_trajectory_bounds("the constant-rate launch (must be outside)", scalar, ref)


def test_update_then_grad_kernel_reads_the_pending_steps_rate(monkeypatch):
    """The single-wave kernel's update-then-grad launch (DDP step path): the pending Adam update it applies first is
    the step after *step_counter - 1 steps."""
    import block5_sched_cases as bc
    from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params

    dims, B = [5, 64, 2], 4
    X, Y, idx, p0 = bc.sized_data(dims, 16, 17, 5)
    P = mlp_num_params(dims)
    k = FusedMLPKernel(dims, bmax=4)
    img = L.window_image()
    res = []
    for lr, tab in ((0.5, _table(img)), (L.f32(L.table_rate(img, 4)), None)):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        g = torch.randn(P + 1, generator=torch.Generator().manual_seed(1)).to(_dev()) * 1e-2
        counter = torch.tensor([5], dtype=torch.int32, device=_dev())  # 5 steps counted, the 5th still pending
        pending = torch.ones(1, dtype=torch.int32, device=_dev())
        cursor = torch.zeros(1, dtype=torch.int32, device=_dev())
        k.train(p, m, v, X, Y, idx, n_items=16, batch=B, steps=1, t0=0, lr=lr, grad_out=g, step_counter=counter,
                cursor=cursor, pending=pending, loss_out=torch.zeros(4, device=_dev()), lr_tab=tab)
        torch.cuda.synchronize()
        res.append((p.cpu(), m.cpu(), v.cpu(), g.cpu()))
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(res[0][0], p0.cpu())


# ---------------------------------------------------------------------------------------------- two ranks, one GPU
@pytest.mark.parametrize("dims,trainers", [([5, 128, 128, 2], ("block5",)), ([5, 64, 2], ("wave_single", "wave_rows"))],
                         ids=["block5", "wave"])
def test_two_ranks_in_kernel_exchange_follow_the_table(dims, trainers, tmp_path):
    """Two ranks sharing the GPU (tests/lr_xg_worker.py, a fresh process: two persistent launches on two streams, the
    bounded spins of the exchange), 70 steps in one launch over a varying window with both ends clamped: the replicas
    are bit-identical, and equal torch DDP + Adam + the same per-step rates at tests/test_xg_block5_gpu.py's
    tolerance (parameter error median < 2e-5, max < 3e-3; losses atol 2e-4, rtol 1e-3)."""
    import os
    import subprocess
    import sys
    import json

    import lr_xg_worker as Wk

    steps, B = 70, 4
    t0w, rates = 3, L.family_window(64)[1]  # 60 entries from step 3: steps 0..2 and 63..69 read the clamped ends
    out = tmp_path / "lrxg.json"
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "lr_xg_worker.py"), str(out), ",".join(map(str, dims)),
                        str(steps), str(B), str(t0w), ",".join(repr(x) for x in rates)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(out.read_text())
    assert res["trainer"] in trainers and res["status"] == [0, 0] and res["steps"] == [steps, steps]
    for key in ("params", "m", "v", "losses"):
        assert res[key][1] == res[key][0], key
    img = L.table_image(t0w, rates)
    step_rates = [L.table_rate(img, k) for k in range(steps)]
    X, Y, shards = Wk.problem()
    net = Wk.net(dims)
    params = list(net.parameters())
    opt = torch.optim.Adam(params, lr=1.0)
    want_l = []
    for s_ in range(steps):
        opt.param_groups[0]["lr"] = step_rates[s_]
        gsum, lsum = [torch.zeros_like(q) for q in params], 0.0
        for sh in shards:
            rows = sh[s_ * B:(s_ + 1) * B]
            loss = F.cross_entropy(net(X[rows]), Y[rows])
            for a, g in zip(gsum, torch.autograd.grad(loss, params)):
                a += g
            lsum += loss.item()
        for q, g in zip(params, gsum):
            q.grad = g / len(shards)
        opt.step()
        want_l.append(lsum / len(shards))
    want = torch.cat([q.detach().reshape(-1) for q in params])
    err = (torch.tensor(res["params"][0]) - want).abs()
    print("  two ranks, %s: parameter error median %.3e max %.3e" % (res["trainer"], err.median(), err.max()))
    assert err.median() < 2e-5 and err.max() < 3e-3
    assert torch.allclose(torch.tensor(res["losses"][0]), torch.tensor(want_l), atol=2e-4, rtol=1e-3)


# ---------------------------------------------------------------------------------------------- (f) the fused engine
@pytest.mark.parametrize("kind", ["epoch", "step"])
@pytest.mark.parametrize("dims", [[5, 64, 2], [5, 128, 128, 2]], ids=["5-64-2", "3x128"])
def test_trainer_fit_fused_engine_follows_the_scheduler(dims, kind):
    """The persistent launches under Trainer.fit, 2 short epochs: the engine stays "fused" (no fallback), and the fit
    matches the torch loop with the same data order, optimizer and scheduler at the tolerances
    tests/test_trainer_gpu.py compares the fused engine with today: |val_loss difference| < 5e-3 (its fused-vs-autograd
    check) and max |dp| < 1e-3 (its DDP-step-vs-persistent check).  The fit without the scheduler is further away."""
    from dct_amd.data.dataset import TensorPairDataset
    from dct_amd.trainer import Trainer

    B, lr, epochs = 4, 0.01, 2
    X, Y = _fit_data(40, 5)

    def fit(k):
        model = _scheduled_model(dims, k, lr)
        t = Trainer(max_epochs=epochs, accelerator="gpu", num_sanity_val_steps=0, verbose=False)
        t.fit(model, DataLoader(TensorPairDataset(X, Y), batch_size=B, shuffle=False),
              DataLoader(TensorPairDataset(X, Y), batch_size=B))
        assert t.engine.name == "fused"
        t.engine.sync_to_model()  # (the flat device parameters into the module: what a checkpoint does)
        return torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters()]), t.callback_metrics["val_loss"]

    got, val = fit(kind)
    want = _torch_fit(dims, kind, lr, X, Y, B, epochs)
    ref = _scheduled_model(dims, "none", lr)
    with torch.no_grad():
        off = 0
        for prm in ref.parameters():
            prm.copy_(want[off: off + prm.numel()].view_as(prm))
            off += prm.numel()
        want_val = float(F.cross_entropy(ref(X), Y))
    plain, _ = fit("none")
    err, gap = float((got - want).abs().max()), float((plain - want).abs().max())
    print("  fused %s %s: max |dp| = %.3e, |dval| = %.3e; without the scheduler max |dp| = %.3e"
          % (dims, kind, err, abs(val - want_val), gap))
    assert err < 1e-3 and abs(val - want_val) < 5e-3
    assert gap > 1e-2
