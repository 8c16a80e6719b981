"""Gradient clipping (norm / value) in the batch-tiled MLP trainer on the GPU (run on a real MI355X): the clamping fold,
the fold_norm + apply kernel pair (csrc/mlp_tile.hip) and the clipped flat SGD step (csrc/optim.hip) element by element
against fp64, the refusals, Trainer(engine="tile").fit and the DDP step path.  Inputs, references and bounds are the
plain case modules': optim_cases (the optimizer step's derived bound), clip_cases ({norm, coef}), wloss_cases, accum_cases."""
import math

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, random_split

import accum_cases as ac
import clip_cases as cc
import optim_cases as oc
import wloss_cases as wc

import dct_amd  # noqa: F401
from dct_amd.data.dataset import TensorPairDataset
from dct_amd.data.synthetic import weather_tensors
from dct_amd.models.mlp import MLPClassifier
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params
from dct_amd.ops.optim import clip_workspace, grad_clip_coef_, sgd_flat_
from dct_amd.trainer import Trainer, seed_everything

pytestmark = pytest.mark.gpu
SEED, DROPOUT = 11, 0.1
# "adam": optimizer="adam" on the launch, AdamW's reference at wd = 0 (which is Adam's)
OPTIMIZERS = {"adam": oc.Hyper("adamw", oc.LR, 0.0, 0.0, False, 0.0, 0.9, 0.999, 1e-8), "adamw": oc.VARIANTS["adamw"],
              "sgd_nest": oc.VARIANTS["sgd_nest"], "sgd_mdw": oc.VARIANTS["sgd_mdw"]}


def tile_depth(n):
    """The additions a squared term passes through in fold_norm + apply: 6 (wave butterfly) + 3 (four wave sums through
    LDS) + ceil(G / 64) (lane l adds partials l, l + 64, ..) + 6 (butterfly), G = ceil((P + 1) / 256) workgroups."""
    return 6 + 3 + -(-(-(-(n + 1) // 256)) // 64) + 6


def _check_clipped_steps(k, case, name, taken, d, cuda, monkeypatch, factors, value=True, off=0, **extra):
    """One grad-mode launch, then train-mode launches from the same state, seed and step word: unclipped, clipped by norm
    at max_norm = factor * the fp64 norm of the grad-mode gradient, clipped by value at the median |g|.  {norm, coef} lie
    inside clip_cases.clip_ref's bound at the new kernels' depth (tile_depth); p / m / v inside optim_cases' derived
    bound of the reference applied to fp32(g * coef_kernel) - the one rounding the kernel makes - or to the exactly
    clamped gradient; every launch reports the grad-mode launch's loss word."""
    dims, B = case
    hp = OPTIMIZERS[name]
    P = mlp_num_params(dims)
    X, Y, idx = (d[key].to(cuda) for key in ("X", "Y", "idx"))
    p0, m0, v0 = oc.state(case, hp, taken)
    kw = dict(optimizer="adam", weight_decay=0.0) if name == "adam" else oc.kernel_args(hp)
    common = dict(n_items=d["idx"].numel() - off, batch=B, steps=1, t0=taken, step_base=taken, dropout=DROPOUT,
                  seed=SEED, lr=oc.LR, **extra)
    gd = torch.full((P + 1,), 7.0, device=cuda)
    k.train(p0.to(cuda), None, None, X, Y, idx[off:], grad_out=gd, clip_val=1e-3, **common)  # (grad mode ignores it)
    g, gloss = gd[:P].cpu(), float(gd[P])

    def train(**clip):
        p, m, v = p0.to(cuda), m0.to(cuda), (None if hp.kind == "sgd" else v0.to(cuda))
        loss = torch.zeros(1, device=cuda)
        k.train(p, m, v, X, Y, idx[off:], loss_out=loss, **kw, **common, **clip)
        torch.cuda.synchronize()
        assert float(loss) == gloss > 0
        return p.cpu(), m.cpu(), None if v is None else v.cpu()

    plain = train()
    monkeypatch.setattr(cc, "clip_depth", tile_depth)
    for fname in factors:
        mn = cc.max_norms(g, 1.0)[fname]
        got = train(clip_val=mn, clip_algorithm="norm")
        norm, coef = k.clip_stats()
        cref = cc.clip_ref(g, 1.0, mn)
        ref = oc.reference(p0, g * np.float32(coef), m0, v0, hp, taken)
        print("%s %s t=%d %s: norm %.6g (ref %.6g) coef %.6g, worst |error| / bound %.4f" % (
            oc.case_id(case), name, taken, fname, norm, cref.norm, coef, oc.excess(got, ref)))
        assert cc.inside(cref, norm, coef), (norm, cref.norm, cref.norm_bound, coef, cref.coef, cref.coef_bound)
        assert oc.inside(got, ref)
        if fname == "inactive":
            assert coef == 1.0
            assert all(a is None or torch.equal(a.nan_to_num(), b.nan_to_num()) for a, b in zip(got, plain))
        elif fname == "active":
            assert coef < 1.0 and not torch.equal(got[0], plain[0])
    if value:
        for q in (0.5, 0.7):  # the median; a gradient that is more than half zeros takes a higher quantile
            c = oc.f32(float(g.abs().double().quantile(q)))
            frac = float((g.abs() > c).float().mean())
            if c > 0 and 0.25 <= frac <= 0.75:
                break
        assert c > 0 and 0.25 <= frac <= 0.75, (c, frac)
        got = train(clip_val=c, clip_algorithm="value")
        ref = oc.reference(p0, g.clamp(-c, c), m0, v0, hp, taken)
        print("%s %s t=%d value: worst |error| / bound %.4f" % (oc.case_id(case), name, taken, oc.excess(got, ref)))
        assert oc.inside(got, ref) and not torch.equal(got[0], plain[0])


@pytest.mark.parametrize("name", list(OPTIMIZERS))
@pytest.mark.parametrize("case", oc.CASES, ids=[oc.case_id(c) for c in oc.CASES])
def test_one_clipped_step_against_fp64(case, name, cuda, monkeypatch):
    k = FusedMLPKernel(case[0], bmax=1024)
    assert math.isnan(k.clip_stats()[0]) and k.clip_stats()[1] == 1.0
    for taken in oc.STEP_COUNTS:
        _check_clipped_steps(k, case, name, taken, wc.inputs(case), cuda, monkeypatch, list(cc.MAX_NORM_FACTORS))


@pytest.mark.parametrize("which", ["weighted", "accumulate", "both"])
def test_norm_clipping_over_weighted_loss_and_accumulation(which, cuda, monkeypatch):
    """Clipping is orthogonal to how the gradient was folded: class weights + smoothing, windows of K = 3 micro-batches
    (the full first window and the short last one), and both together."""
    dims, B, K = acase = ac.CASES[1]
    w, eps = ac.variant_args("ws", dims[-1])
    wl = dict(class_weight=w.to(cuda), label_smoothing=eps) if which != "accumulate" else {}
    acc = dict(accumulate=K) if which != "weighted" else {}
    d, offs = (ac.inputs(acase), [win * K * B for win in ac.windows(acase)]) if acc else (wc.inputs((dims, B)), (0, 2 * B))
    k = FusedMLPKernel(dims, bmax=1024)
    for off in offs:
        for name, taken in (("sgd_nest", 0), ("adamw", 3)):
            _check_clipped_steps(k, (dims, B), name, taken, d, cuda, monkeypatch, ["active"], False, off, **wl, **acc)


def test_refusals_and_the_plan(cuda):
    dims, B = case = oc.CASES[1]
    d = wc.inputs(case)
    X, Y, idx, p = (d[key].to(cuda) for key in ("X", "Y", "idx", "p"))
    m, v, losses = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(4, device=cuda)
    args = dict(n_items=d["idx"].numel(), steps=1, t0=0, lr=oc.LR, loss_out=losses)
    tile = FusedMLPKernel(dims, bmax=1024)
    assert all(tile.plan.trainer(b, clipped=True) == "tile" for b in (1, 16, 17, 1024))
    assert tile.plan.trainer(1025, clipped=True) == "none"
    assert native().MlpPlan([5, 300, 2], 16).trainer(4, clipped=True) == "none"
    with pytest.raises(ValueError, match="batch-tiled"):
        FusedMLPKernel(dims, bmax=4).train(p, m, v, X, Y, idx, batch=4, clip_val=0.5, **args)
    ws = tile._tile_args(p.device, B)
    small = torch.zeros(64, device=cuda)
    for bad in (dict(clip_kind=3, clip_val=0.5), dict(clip_kind=-1, clip_val=0.5), dict(clip_kind=2, clip_val=0.0),
                dict(clip_kind=2, clip_val=-0.5), dict(clip_kind=1, clip_val=float("inf")),
                dict(clip_kind=1, clip_val=float("nan")), dict(clip_kind=1, clip_val=0.5),  # norm without a workspace
                dict(clip_kind=1, clip_val=0.5, clip_ws=small.data_ptr(), clip_ws_floats=64)):
        with pytest.raises((ValueError, RuntimeError)):
            tile.plan.train(p.data_ptr(), m.data_ptr(), v.data_ptr(), 0, X.data_ptr(), X.stride(0), Y.data_ptr(),
                            idx.data_ptr(), args["n_items"], B, 1, 0, oc.LR, 0.9, 0.999, 1e-8, 0.0, 0.0, 0, 0,
                            losses.data_ptr(), 0, 0, 0, 0, **ws, **bad)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), d["p"]) and not any(bool(t.any()) for t in (m, v, losses, small))  # nothing written
    tile.train(p, m, v, X, Y, idx, batch=B, clip_val=0.5, **args)  # and the launch that is right does run
    torch.cuda.synchronize()
    assert not torch.equal(p.cpu(), d["p"]) and float(losses[0]) > 0 and math.isfinite(tile.clip_stats()[0])


@pytest.mark.parametrize("algorithm", ["norm", "value"])
@pytest.mark.parametrize("variant", ["sgd_m", "sgd_nest"])
@pytest.mark.parametrize("n", [1027, 5])
def test_flat_sgd_step_clipped(n, variant, algorithm, cuda):
    """dct_sgd_flat_step_clipped with the host step count and with the device counter, against optim_cases.reference on
    the fp64-clipped gradient; by norm the coefficient's own error (clip_ref's eps_c, and the product's rounding) joins
    the bound as clip_cases.clipped_adam_ref does it for flat Adam.  Guard words stay, g is not rewritten."""
    hp = oc.VARIANTS[variant]
    for taken in oc.STEP_COUNTS:
        for device_counter in (False, True):
            gen = torch.Generator().manual_seed(100 + n + taken)
            p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.05
            m0 = torch.randn(n, generator=gen) * (1e3 if taken == 0 else 0.05)
            bufs = [torch.cat([t, torch.tensor([123.0])]).to(cuda) for t in (p0, g0, m0)]
            p, g, m = (b[:n] for b in bufs)
            counter = torch.full((1,), taken + 1, dtype=torch.int32, device=cuda) if device_counter else None
            if algorithm == "norm":
                mn = cc.max_norms(g0, 1.0)["active"]
                clip = dict(clip_coef=grad_clip_coef_(g, mn, clip_workspace(cuda))[1:])
                cref = cc.clip_ref(g0, 1.0, mn)
                at = lambda c: oc.reference(p0, g0.double() * c, m0, None, hp, taken)  # noqa: E731
                ref, rel = at(cref.coef), cref.eps_c + oc.U
                ends = [at(cref.coef * (1 - rel)), at(cref.coef * (1 + rel))]
                ref = ref._replace(p_bound=ref.p_bound + 2 * torch.maximum(*[(r.p - ref.p).abs() for r in ends]),
                                   m_bound=ref.m_bound + 2 * torch.maximum(*[(r.m - ref.m).abs() for r in ends]))
            else:
                c = oc.f32(float(g0.abs().median()))
                clip, ref = dict(clip_value=c), oc.reference(p0, g0.clamp(-c, c), m0, None, hp, taken)
            # (with a counter the host count is ignored: it is handed a wrong one)
            sgd_flat_(p, g, m, 5 - 4 * bool(taken) if device_counter else taken + 1, oc.LR, hp.momentum, hp.dampening,
                      hp.nesterov, hp.wd, step_counter=counter, **clip)
            torch.cuda.synchronize()
            assert all(float(b[n]) == 123.0 for b in bufs) and torch.equal(g.cpu(), g0)
            got = (p.cpu(), m.cpu(), None)
            assert oc.inside(got, ref), (taken, device_counter, oc.excess(got, ref))
            assert not oc.inside(got, oc.reference(p0, g0, m0, None, hp, taken))  # (the clip acted)


@pytest.mark.parametrize("algorithm,val", [("norm", 0.05), ("value", 0.002)])
@pytest.mark.parametrize("opt", ["adam", "sgd"])
@pytest.mark.parametrize("B", [4, 40])
def test_trainer_fit_engine_tile(B, opt, algorithm, val):
    """Trainer(engine="tile", gradient_clip_val=v).fit on the GPU against the CPU autograd fit of the same seed, inside
    test_optim_gpu.py::test_trainer_fit_on_the_fused_engine's thresholds; the clip acts on the CPU run's last step."""
    kw = dict(optimizer="sgd", momentum=0.9, nesterov=True) if opt == "sgd" else {}
    steps = 7
    n_train, n_val = (steps - 1) * B + 3, 50

    def fit(acc, engine):
        seed_everything(42)
        x, y = weather_tensors(n_train + n_val, seed=0)
        tr, va = random_split(TensorPairDataset(x, y), [n_train, n_val])
        torch.manual_seed(0)
        model = MLPClassifier(5, (64,), dropout=0, **kw)
        t = Trainer(max_epochs=1, accelerator=acc, engine=engine, logger=None, num_sanity_val_steps=0, verbose=False,
                    gradient_clip_val=val, gradient_clip_algorithm=algorithm)
        t.fit(model, DataLoader(tr, batch_size=B, shuffle=True), DataLoader(va, batch_size=B))
        return t, torch.cat([q.detach().reshape(-1).cpu() for q in model.parameters()])

    c, want = fit("cpu", "auto")
    assert c.engine.name == "autograd" and c.global_step == steps
    if algorithm == "norm":
        assert c.engine.grad_clip_stats()[1] < 1.0
    else:
        assert max(float(q.grad.abs().max()) for q in c.engine.params) >= val * (1 - 1e-6)
    t, _ = fit("gpu", "tile")
    eng = t.engine
    assert eng.name == "fused" and eng.kernel.plan.use_tile and eng.kernel.plan.trainer(B, clipped=True) == "tile"
    assert t.global_step == eng.global_step == steps == int(eng.step_counter.item())
    norm, coef = eng.grad_clip_stats()
    assert (math.isfinite(norm) and 0 < coef < 1) if algorithm == "norm" else (math.isnan(norm) and coef == 1.0)
    err = (eng.p.cpu() - want).abs()
    print("%s %s B %d: param err median %.3e max %.3e" % (opt, algorithm, B, err.median(), err.max()))
    assert err.median() < 1e-5 and err.max() < 2e-3


@pytest.mark.parametrize("kind,algorithm,val", [("sgd", "norm", 0.05), ("adamw", "norm", 0.05), ("sgd", "value", 0.002)])
@pytest.mark.parametrize("graph", ["1", "0"])
def test_clipped_ddp_step_path_world1_matches_persistent(graph, kind, algorithm, val, monkeypatch):
    """DCT_FORCE_DDP=1 at world size 1 (grad-mode launch -> one-rank all-reduce -> [norm kernel ->] clipped flat SGD /
    flat Adam with decoupled decay, HIP-graph chunks of 7) reproduces the clipped train-mode launches over 39 steps;
    structure and tolerances of test_optim_gpu.py::test_ddp_step_path_world1_matches_persistent."""
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
        eng = FusedMLPEngine(model, init_distributed("gpu"), B, seed=42, gradient_clip_val=val,
                             gradient_clip_algorithm=algorithm, adam=optim_hparams_of(model.configure_optimizers()))
        assert eng.kernel.plan.use_tile and not eng.fused_update and eng.xg is None and eng.gx is None
        eng.attach_data(x, y, rows[:n_train], rows[n_train:])
        n = eng.upload_epoch_indices(0)
        loss = torch.zeros(64, device=eng.device)
        eng.run_steps(n, 20, loss, first_step=0)
        eng.run_steps(n, 19, loss, first_step=20)
        torch.cuda.synchronize()
        assert int(eng.step_counter.item()) == steps
        return eng.p.cpu(), eng.m.cpu(), loss[:steps].cpu(), eng

    p0, m0, l0, e0 = run("0")
    p1, m1, l1, e1 = run("1")
    assert e0.step_mode == "fused-persistent" and e1.ddp and e1.comm is not None and e1.graph_used == (graph == "1")
    if algorithm == "norm":
        assert 0 < e0.grad_clip_stats()[1] < 1 and 0 < e1.grad_clip_stats()[1] < 1  # the clip acts on the last step
    assert torch.allclose(l0, l1, atol=1e-4), (l0 - l1).abs().max()
    assert (p0 - p1).abs().max() < 1e-3 and (p0 - p1).abs().median() < 1e-5
    assert torch.allclose(m0, m1, atol=1e-4) and bool(m0.any())
