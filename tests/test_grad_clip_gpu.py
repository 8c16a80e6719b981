"""Gradient clipping on the GPU against the fp64 references and counted bounds of tests/clip_cases.py: the norm kernel
(dct_grad_clip_coef), the flat Adam step that reads its coefficient or clamps by value (dct_adam_flat_step_clipped),
and both engines, every step checked from the unclipped gradient the step leaves in memory (the clip is applied inside
Adam; flat_g / eng.g is not rewritten), so the run-to-run noise of the split-K atomics cannot enter a comparison.
Every test prints its worst error / bound ratio before it asserts.

Measured on an MI355X (2026-10-20), worst error / bound over every case: norm 0.11, coef 0.14; p 0.998 (its own final
rounding, u |p|, is most of that bound), m 0.43, v 0.44.  A coefficient of exactly 1.0 and a null coefficient both
reproduce dct_adam_flat_step bit for bit, and the graph engine at max_norm = 1e30 the DCT_DW_INTO_ADAM=0 step."""
import functools
import math

import pytest
import torch

import clip_cases as K
import wide_step_cases as C

pytestmark = pytest.mark.gpu

SEED = 11
GUARD = 123.0


def _nat():
    from dct_amd.ops._native import native

    return native()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _ratio(what, got, want, bound):
    got = got.double().cpu()
    if not bool(torch.isfinite(got).all()):
        print("  %s: non-finite values" % what)
        return float("inf")
    r = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
    print("  %s: worst error / bound %.4f" % (what, r))
    return r


@functools.lru_cache(maxsize=None)
def _case(n, scale):
    """p, g, m, v on the CPU; g with the slot past n (PAST_N)."""
    return K.clip_inputs(n, scale, SEED, slot=True)


class Ws:
    """The norm kernel's words: {norm, coef, ticket, pad, partials}, zeroed once."""

    def __init__(self):
        self.t = torch.zeros(4 + _nat().grad_clip_workspace_floats(), dtype=torch.float32, device=_dev())

    def launch(self, g, n, gs, mn):
        _nat().grad_clip_coef(g.data_ptr(), n, gs, mn, self.t[4:].data_ptr(), self.t[2:].data_ptr(), self.t.data_ptr(),
                              _st())

    def stats(self):
        torch.cuda.synchronize()
        assert int(_bits(self.t[2:3]).item()) == 0, "the ticket was not reset"
        return self.t[:2].clone()

    @property
    def coef_ptr(self):
        return self.t[1:].data_ptr()


# ---------------------------------------------------------------------------------------------- (a) the norm kernel
def test_workspace_matches_the_case_tables():
    assert _nat().grad_clip_workspace_floats() == K.CLIP_MAX_GRID


@pytest.mark.parametrize("n", list(K.CLIP_NS))
def test_norm_and_coef_inside_bounds_and_bit_stable(n):
    worst = 0.0
    for scale in K.CLIP_SCALES:
        g_cpu = _case(n, scale)[1]
        g = g_cpu.to(_dev())
        for gs in (1.0, 0.125):
            for name, mn in K.max_norms(g_cpu[:n], gs).items():
                ref = K.clip_ref(g_cpu[:n], gs, mn)
                ws = Ws()
                ws.launch(g, n, gs, mn)
                first = ws.stats()
                ws.launch(g, n, gs, mn)
                second = ws.stats()
                norm, coef = first.tolist()
                rn, rc = K.ratio(norm - ref.norm, ref.norm_bound), K.ratio(coef - ref.coef, ref.coef_bound)
                print("  n %d %s gs %g %s: norm %.9g (error / bound %.3f) coef %.9g (%.3f)"
                      % (n, scale, gs, name, norm, rn, coef, rc))
                worst = max(worst, rn, rc)
                assert rn <= 1.0 and rc <= 1.0, (n, scale, gs, name, norm, ref.norm, coef, ref.coef)
                assert _same_bits(first, second), "two launches on one input differ"
                if name == "inactive":
                    assert coef == 1.0
                # the slot past n was not read: with it the norm would be ~PAST_N
                assert norm < 0.9 * K.PAST_N
        assert float(g[n]) == K.PAST_N and _same_bits(g[:n], g_cpu[:n].to(_dev()))
    print("worst error / bound: %.3f" % worst)


def test_norm_kernel_replays_in_a_graph_with_the_same_bits():
    n = K.CLIP_N_TWO_PASSES
    g_cpu = _case(n, "tabular")[1]
    g = g_cpu.to(_dev())
    mn = K.max_norms(g_cpu[:n], 1.0)["active"]
    ws = Ws()
    ws.launch(g, n, 1.0, mn)
    eager = ws.stats()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(_dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
            ws.launch(g, n, 1.0, mn)
    torch.cuda.current_stream().wait_stream(s)
    for k in range(3):
        ws.t[:2].fill_(float("nan"))
        graph.replay()
        assert _same_bits(ws.stats(), eager), "replay %d differs from the eager launch" % k
    ref = K.clip_ref(g_cpu[:n], 1.0, mn)
    assert K.inside(ref, *eager.tolist())


def test_launcher_rejects_bad_arguments():
    ws = Ws()
    g = torch.zeros(8, device=_dev())
    for args in ((g.data_ptr(), 0, 1.0, 1.0), (g.data_ptr(), 8, 1.0, -1.0), (g.data_ptr(), 8, 1.0, float("nan")),
                 (g[1:].data_ptr(), 4, 1.0, 1.0), (0, 8, 1.0, 1.0)):
        with pytest.raises(Exception):
            _nat().grad_clip_coef(*args, ws.t[4:].data_ptr(), ws.t[2:].data_ptr(), ws.t.data_ptr(), _st())
    with pytest.raises(Exception):
        _nat().adam_flat_step_clipped(g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), 0, 8, 1e-3, 0.9, 0.999,
                                      1e-8, 0.0, 1, 1.0, 0, 0, 0, 0, 0, 0, 0, -1.0, _st())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- (b) clipped Adam
class State:
    """p, g, m, v on the device: p, m, v with a guard element after n, g with the slot past n."""

    def __init__(self, n, scale):
        p, g, m, v = _case(n, scale)
        self.n, self.scale = n, scale
        self.cpu = (p, g[:n], m, v)
        guard = torch.full((1,), GUARD)
        self.init = [torch.cat([p, guard]).to(_dev()), g.to(_dev()), torch.cat([m, guard]).to(_dev()),
                     torch.cat([v, guard]).to(_dev())]
        self.reset()

    def reset(self):
        self.p, self.g, self.m, self.v = (x.clone() for x in self.init)
        self.pb = torch.full((self.n + 1,), -7.0, dtype=torch.bfloat16, device=_dev())

    def adam(self, hp, t, step, coef_ptr=0, clip_value=0.0, clipped=True):
        sc = 0 if step is None else step.data_ptr()
        args = (self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.pb.data_ptr(), self.n,
                hp.lr, hp.b1, hp.b2, hp.eps, hp.wd, t if step is None else 1, hp.grad_scale, hp.decoupled, sc, 0, 0, 0, 0)
        if clipped:
            _nat().adam_flat_step_clipped(*args, coef_ptr, clip_value, _st())
        else:
            _nat().adam_flat_step(*args, _st())
        torch.cuda.synchronize()

    def result(self):
        return self.p.clone(), self.m.clone(), self.v.clone(), self.pb.clone()

    def check(self, what, ref):
        n = self.n
        assert _same_bits(self.g, self.init[1]), what + ": g was rewritten"
        for x in (self.p, self.m, self.v):
            assert float(x[n]) == GUARD, what + ": wrote past n"
        assert float(self.pb[n]) == -7.0
        rp = _ratio(what + " p", self.p[:n], ref.p, ref.p_bound)
        rm = _ratio(what + " m", self.m[:n], ref.m, ref.m_bound)
        rv = _ratio(what + " v", self.v[:n], ref.v, ref.v_bound)
        assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0, (what, rp, rm, rv)
        assert torch.equal(self.pb[:n], self.p[:n].to(torch.bfloat16)), what + ": bf16 shadow != bf16(p)"


def _step_tensor(t):
    return torch.tensor([t], dtype=torch.int32, device=_dev())


@functools.lru_cache(maxsize=None)
def _clip_ref(n, scale, grad_scale, name):
    """(max_norm, its fp64 reference) of a case: computed once, shared by every launch of the case."""
    g = _case(n, scale)[1][:n]
    mn = K.max_norms(g, grad_scale)[name]
    return mn, K.clip_ref(g, grad_scale, mn)


def _norm_case(s, hp, t, dc, name):
    """The norm kernel, then the clipped Adam launch that reads its coefficient: stats and p, m, v inside the bounds;
    for "inactive" the coefficient is exactly 1.0 and the result the unclipped launch's, bit for bit."""
    p, g, m, v = s.cpu
    n = s.n
    mn, cref = _clip_ref(n, s.scale, hp.grad_scale, name)
    step = (lambda: _step_tensor(t)) if dc else (lambda: None)
    s.reset()
    ws = Ws()
    ws.launch(s.g, n, hp.grad_scale, mn)
    s.adam(hp, t, step(), coef_ptr=ws.coef_ptr)
    norm, coef = ws.stats().tolist()
    assert K.inside(cref, norm, coef), (n, name, norm, cref.norm, coef, cref.coef)
    what = "n %d %s wd %g gs %g dec %d t %d %s" % (n, name, hp.wd, hp.grad_scale, hp.decoupled, t,
                                                   "device counter" if dc else "host t")
    s.check(what, K.clipped_adam_ref(p, g, m, v, t, hp, cref, device_counter=dc))
    if name == "inactive":
        assert coef == 1.0
        got = s.result()
        s.reset()
        s.adam(hp, t, step(), clipped=False)
        assert all(_same_bits(a.float(), b.float()) for a, b in zip(got, s.result())), \
            what + ": coef == 1.0 differs from the unclipped launch"
    elif name == "active":
        assert coef < 1.0


@pytest.mark.parametrize("counter", ["host_t", "device_counter"])
@pytest.mark.parametrize("n", list(K.CLIP_NS))
def test_adam_clipped_by_norm_inside_widened_bounds(n, counter):
    """Every size x scale x max_norm of the case tables, every Hyper, t in {1, 10}."""
    for scale in K.CLIP_SCALES:
        s = State(n, scale)
        for hp in K.CLIP_HYPERS:
            for name in K.MAX_NORM_FACTORS:
                for t in K.CLIP_STEPS:
                    _norm_case(s, hp, t, counter == "device_counter", name)


@pytest.mark.parametrize("counter", ["host_t", "device_counter"])
def test_adam_clipped_by_norm_takes_a_second_grid_stride_pass(counter):
    """Past Adam's own 2048 workgroups of 256 float4s (the 3.4 M-parameter tabular model's launch): 300 float4s of a
    second pass, tail 3."""
    s = State(K.CLIP_ADAM_N_TWO_PASSES, K.CLIP_ADAM_BIG_SCALE)
    for name in K.MAX_NORM_FACTORS:
        _norm_case(s, K.CLIP_ADAM_BIG_HYPER, 10, counter == "device_counter", name)


@pytest.mark.parametrize("counter", ["host_t", "device_counter"])
@pytest.mark.parametrize("n", list(K.CLIP_NS))
def test_adam_with_a_null_coefficient_is_the_unclipped_launch_bit_for_bit(n, counter):
    dc = counter == "device_counter"
    for scale in K.CLIP_SCALES:
        s = State(n, scale)
        for hp in K.CLIP_HYPERS:
            for t in K.CLIP_STEPS:
                step = (lambda: _step_tensor(t)) if dc else (lambda: None)
                s.reset()
                s.adam(hp, t, step(), clipped=False)
                want = s.result()
                s.reset()
                s.adam(hp, t, step())  # null coefficient, no clamp
                assert all(_same_bits(a.float(), b.float()) for a, b in zip(s.result(), want)), "null clip differs"


def _value_case(s, hp, t, dc):
    p, g, m, v = s.cpu
    c = K.value_clip(g, hp.grad_scale)
    s.reset()
    s.adam(hp, t, _step_tensor(t) if dc else None, clip_value=c)
    what = "value n %d wd %g dec %d t %d %s" % (s.n, hp.wd, hp.decoupled, t, "device counter" if dc else "host t")
    s.check(what, K.value_adam_ref(p, g, m, v, t, hp, c, device_counter=dc))


@pytest.mark.parametrize("counter", ["host_t", "device_counter"])
@pytest.mark.parametrize("n", list(K.CLIP_NS) + [K.CLIP_ADAM_N_TWO_PASSES])
def test_adam_clipped_by_value_inside_bounds(n, counter):
    big = n == K.CLIP_ADAM_N_TWO_PASSES
    for scale in ([K.CLIP_ADAM_BIG_SCALE] if big else K.CLIP_SCALES):
        s = State(n, scale)
        for wd, dec in (((0.05, 0),) if big else ((0.0, 0), (0.05, 0), (0.05, 1))):
            hp = C.Hyper(C.LR, C.B1, C.B2, C.EPS, wd, K.VALUE_GRAD_SCALE, dec)
            for t in ([10] if big else K.CLIP_STEPS):
                _value_case(s, hp, t, counter == "device_counter")


# ---------------------------------------------------------------------------------------------- (c) AutogradEngine
TT_B = 128


def _tt_data(n=2048, f=64, seed=3):
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(n, f, generator=gen)
    Y = ((X[:, : f // 2].sum(1) - X[:, f // 2:].sum(1)) > 0).long()
    return X, Y


def _tt_engine(**clip):
    from dct_amd.models.tabtransformer import TabTransformer
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import AutogradEngine
    from dct_amd.trainer.trainer import seed_everything

    ctx = init_distributed("gpu")
    seed_everything(7)
    m = TabTransformer(num_features=64, d_model=64, heads=4, layers=2, lr=3e-3)
    eng = AutogradEngine(m, ctx, TT_B, seed=7, **clip)
    X, Y = _tt_data()
    rows = torch.randperm(2048, generator=torch.Generator().manual_seed(1))
    eng.attach_data(X.to(_dev()), Y.to(_dev()), rows[:1792], rows[1792:])
    return eng


@functools.lru_cache(maxsize=None)
def _first_norm():
    """The gradient norm of the first step (an unclipped eager step of the same model and batch)."""
    eng = _tt_engine()
    eng.train_step(eng.train_rows[:TT_B].to(_dev()), 0)
    torch.cuda.synchronize()
    return float(eng.flat_g.double().norm())


def _hyper(opt):
    g = opt.param_groups[0]
    return C.Hyper(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], 1.0, 0)


def _check_engine_step(what, before, after, g, t, hp, clip_val, algorithm, stats):
    """One step from what it left in memory: ``before`` / ``after`` = (p, m, v), ``g`` the unclipped gradient."""
    p0, m0, v0 = (x.cpu() for x in before)
    g = g.cpu()
    if algorithm == "norm":
        cref = K.clip_ref(g, 1.0, clip_val)
        norm, coef = stats
        rn, rc = K.ratio(norm - cref.norm, cref.norm_bound), K.ratio(coef - cref.coef, cref.coef_bound)
        print("  %s: norm %.6g (error / bound %.3f) coef %.6g (%.3f)" % (what, norm, rn, coef, rc))
        assert rn <= 1.0 and rc <= 1.0, (what, norm, cref.norm, coef, cref.coef)
        ref = K.clipped_adam_ref(p0, g, m0, v0, t, hp, cref, device_counter=True)
    else:
        cref = None
        ref = K.value_adam_ref(p0, g, m0, v0, t, hp, clip_val, device_counter=True)
    rp = _ratio(what + " p", after[0], ref.p, ref.p_bound)
    rm = _ratio(what + " m", after[1], ref.m, ref.m_bound)
    rv = _ratio(what + " v", after[2], ref.v, ref.v_bound)
    assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0, (what, rp, rm, rv)
    # and the step did clip: the unclipped update is outside
    plain = C.adam_ref(p0, g, m0, v0, t, hp, device_counter=True)
    assert bool(((plain.m - ref.m).abs() > ref.m_bound).any())
    return cref


def _run_autograd(steps, clip_val, algorithm, device_loop=False):
    eng = _tt_engine(gradient_clip_val=clip_val, gradient_clip_algorithm=algorithm)
    opt = eng.optimizer
    hp = _hyper(opt)
    rows_dev = eng.train_rows.to(_dev())
    loss = torch.zeros(steps, device=_dev())
    coefs = []
    for s in range(steps):
        torch.cuda.synchronize()
        before = tuple(x.clone() for x in (eng.flat_p, opt.m, opt.v))
        if device_loop:
            eng.run_device_steps(rows_dev, s, 1, loss)
        else:
            eng.train_step(rows_dev[s * TT_B:(s + 1) * TT_B], s)
        torch.cuda.synchronize()
        assert opt.step_count == s + 1
        cref = _check_engine_step("step %d" % (s + 1), before, (eng.flat_p, opt.m, opt.v), eng.flat_g, s + 1, hp,
                                  clip_val, algorithm, eng.grad_clip_stats())
        coefs.append(cref.coef if cref else None)
    return eng, coefs


def test_autograd_engine_eager_steps_clip_by_norm(monkeypatch):
    monkeypatch.setenv("DCT_GRAPH", "0")
    eng, coefs = _run_autograd(3, 0.5 * _first_norm(), "norm")
    assert not eng.graph_used and coefs[0] == pytest.approx(0.5, rel=1e-2)


def test_autograd_engine_replayed_steps_clip_by_norm(monkeypatch):
    monkeypatch.setenv("DCT_GRAPH", "1")
    from dct_amd.trainer.engines import AutogradEngine

    eng, coefs = _run_autograd(AutogradEngine.GRAPH_WARMUP + 3, 0.5 * _first_norm(), "norm")
    assert eng.graph_used and eng.last_step_mode == "replayed"
    assert all(c < 1.0 for c in coefs[-3:])  # the three replayed steps clip


def test_autograd_engine_device_loop_clips_by_norm(monkeypatch):
    monkeypatch.setenv("DCT_GRAPH", "1")
    from dct_amd.trainer.engines import AutogradEngine

    eng, _ = _run_autograd(AutogradEngine.GRAPH_WARMUP + 2, 0.5 * _first_norm(), "norm", device_loop=True)
    assert eng.graph_used and getattr(eng, "_dgraph", None) is not None


def test_autograd_engine_clips_after_the_reducer(monkeypatch):
    monkeypatch.setenv("DCT_GRAPH", "1")
    from dct_amd.trainer.engines import AutogradEngine

    norm0 = _first_norm()
    monkeypatch.setenv("DCT_FORCE_DDP", "1")  # a one-rank communicator and the bucket reducer
    eng, _ = _run_autograd(AutogradEngine.GRAPH_WARMUP + 2, 0.5 * norm0, "norm")
    assert eng.reducer is not None and eng.graph_used


def test_autograd_engine_clips_by_value(monkeypatch):
    monkeypatch.setenv("DCT_GRAPH", "1")
    from dct_amd.trainer.engines import AutogradEngine

    eng = _tt_engine()
    eng.train_step(eng.train_rows[:TT_B].to(_dev()), 0)
    torch.cuda.synchronize()
    c = float(eng.flat_g.abs().median())  # about half of the elements clamped
    eng, _ = _run_autograd(AutogradEngine.GRAPH_WARMUP + 2, c, "value")
    assert eng.graph_used and eng.grad_clip_stats()[1] == 1.0


# ---------------------------------------------------------------------------------------------- (d) GraphMLPEngine
G_DIMS, G_B = [64, 256, 256, 2], 64


def _graph_engine(monkeypatch, dw_into_adam, **clip):
    from dct_amd.models.mlp import MLPClassifier
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import adam_hparams_from
    from dct_amd.trainer.graph_engine import GraphMLPEngine

    monkeypatch.setenv("DCT_DW_INTO_ADAM", dw_into_adam)
    torch.manual_seed(0)
    model = MLPClassifier(G_DIMS[0], hidden=tuple(G_DIMS[1:-1]), num_classes=G_DIMS[-1], dropout=0.0, loss="ce", lr=1e-3)
    eng = GraphMLPEngine(model, init_distributed("gpu"), G_B, seed=42,
                         adam=adam_hparams_from(model.configure_optimizers()), use_graph=False, **clip)
    gen = torch.Generator().manual_seed(0)
    X = torch.randn(4 * G_B, G_DIMS[0], generator=gen)
    Y = ((X @ torch.randn(G_DIMS[0], generator=gen)) > 0).long()
    rows = torch.arange(4 * G_B)
    eng.attach_data(X, Y, rows, rows[:G_B])
    eng.idx[:G_B].copy_(torch.arange(G_B, dtype=torch.int32))
    return eng


def _graph_step(eng, rows):
    """One step on the first ``rows`` rows; (p, m, v) before, and the step's loss."""
    before = tuple(x.clone() for x in (eng.p, eng.m, eng.v))
    loss_out = torch.zeros(1, device=_dev())
    eng.cursor.zero_()
    eng._step(rows, loss_out, rows)
    torch.cuda.synchronize()
    assert int(eng.step_counter.item()) == 1 and math.isfinite(float(loss_out.item()))
    return before


def _graph_hyper(eng):
    a = eng.adam
    return C.Hyper(a["lr"], a["betas"][0], a["betas"][1], a["eps"], a["weight_decay"], 1.0, 0)


def test_graph_engine_with_coef_one_is_the_g_path_bit_for_bit(monkeypatch):
    plain = _graph_engine(monkeypatch, "0")
    _graph_step(plain, G_B)
    clipped = _graph_engine(monkeypatch, "1", gradient_clip_val=1e30)
    assert clipped.exe.partial_layers == 0  # every dW accumulates into g, whatever DCT_DW_INTO_ADAM says
    _graph_step(clipped, G_B)
    norm, coef = clipped.grad_clip_stats()
    assert coef == 1.0 and norm == pytest.approx(float(clipped.g[: clipped.P].double().norm()), rel=1e-5)
    for a, b in ((plain.p, clipped.p), (plain.m, clipped.m), (plain.v, clipped.v), (plain.g, clipped.g)):
        assert _same_bits(a, b)
    assert torch.equal(plain.p_bf16, clipped.p_bf16)


@pytest.mark.parametrize("rows", [G_B, 37])
def test_graph_engine_clips_by_the_norm_of_the_parameters_alone(monkeypatch, rows):
    probe = _graph_engine(monkeypatch, "0")
    _graph_step(probe, rows)
    clip_val = 0.25 * float(probe.g[: probe.P].double().norm())
    eng = _graph_engine(monkeypatch, "1", gradient_clip_val=clip_val)
    before = _graph_step(eng, rows)
    P = eng.P
    g = eng.g.cpu()
    assert float(g[P]) > 0.1  # the loss slot holds the batch loss
    stats = eng.grad_clip_stats()
    cref = _check_engine_step("graph engine rows %d" % rows, before, (eng.p, eng.m, eng.v), g[:P], 1, _graph_hyper(eng),
                              clip_val, "norm", stats)
    assert cref.coef == pytest.approx(0.25, rel=1e-2)
    with_slot = K.clip_ref(g[: P + 1], 1.0, clip_val)
    assert not K.inside(with_slot, *stats), "the norm cannot tell whether it read the loss slot"
    assert torch.equal(eng.p_bf16, eng.p.to(torch.bfloat16))


def test_graph_engine_clips_by_value(monkeypatch):
    probe = _graph_engine(monkeypatch, "0")
    _graph_step(probe, G_B)
    c = float(probe.g[: probe.P].abs().median())
    assert c > 0.0
    eng = _graph_engine(monkeypatch, "1", gradient_clip_val=c, gradient_clip_algorithm="value")
    before = _graph_step(eng, G_B)
    _check_engine_step("graph engine by value", before, (eng.p, eng.m, eng.v), eng.g[: eng.P], 1, _graph_hyper(eng), c,
                       "value", eng.grad_clip_stats())


def test_trainer_routes_a_clipped_small_mlp_around_the_fused_engine():
    from torch.utils.data import DataLoader, TensorDataset

    from dct_amd.models.mlp import MLPClassifier
    from dct_amd.trainer import Trainer

    gen = torch.Generator().manual_seed(0)
    X = torch.randn(1024, 64, generator=gen)
    Y = (X[:, 0] > 0).long()
    model = MLPClassifier(64, hidden=(128, 128), dropout=0.0, loss="mse", lr=1e-3)
    tl, vl = DataLoader(TensorDataset(X, Y), batch_size=256), DataLoader(TensorDataset(X[:256], Y[:256]), batch_size=256)
    tr = Trainer(max_epochs=1, accelerator="gpu", verbose=False, num_sanity_val_steps=0, gradient_clip_val=0.05)
    tr.fit(model, tl, vl)
    assert tr.engine.name == "graph" and tr.engine.exe.partial_layers == 0
    norm, coef = tr.engine.grad_clip_stats()
    assert norm > 0.0 and 0.0 < coef <= 1.0
    with pytest.raises(RuntimeError, match="cannot clip"):
        Trainer(max_epochs=1, accelerator="gpu", engine="fused", verbose=False, num_sanity_val_steps=0,
                gradient_clip_val=0.05).fit(model, tl, vl)
