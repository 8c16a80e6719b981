"""The skip connection (residual=True) and RMSNorm (norm="rms") of the batch-tiled MLP trainer and inference kernel on
the GPU against torch fp64 autograd on the CPU under the host dropout masks.  Measure, limit and LIMIT's rule are
test_tile_norm_gpu.py's (LIMIT x torch fp32's own error on the case); the ratios are in profiles/tile_res_cost.log."""
import pytest
import torch
import torch.nn.functional as F

from dct_amd.ops.fused_mlp import FusedMLPKernel, activation_fn, dropout_keep_mask, mlp_num_params

pytestmark = pytest.mark.gpu

LIMIT = 8.0
P_DROP, SEED = 0.2, 11
WORDS = {None: "", "layer": "gb", "rms": "g"}  # the norm's vectors per hidden layer


def _case(dims, n, norm, seed=1, const_b0=None):
    """Flat parameters in the kernels' order - all linears, then the norm's words of the hidden layers - and data."""
    g = torch.Generator().manual_seed(seed)
    parts = [t for i, o in zip(dims[:-1], dims[1:])
             for t in (torch.randn(o * i, generator=g) / i ** 0.5, torch.randn(o, generator=g) * 0.1)]
    if const_b0 is not None:
        parts[1] = torch.full_like(parts[1], const_b0)
    for h in dims[1:-1]:
        parts += [0.5 + torch.rand(h, generator=g) if w == "g" else torch.randn(h, generator=g) * 0.1 for w in WORDS[norm]]
    return torch.cat(parts), torch.randn(n, dims[0], generator=g), torch.randint(0, dims[-1], (n,), generator=g)


def _leaves(flat, dims, dt, norm):
    shapes = [s for i, o in zip(dims[:-1], dims[1:]) for s in ((o, i), (o,))] + [(h,) for h in dims[1:-1] for _ in WORDS[norm]]
    parts = flat.split([s[0] * (s[1] if len(s) == 2 else 1) for s in shapes])
    return [t.view(s).to(dt).requires_grad_() for t, s in zip(parts, shapes)]


def _forward(leaves, x, L, kind, gstep, norm, res):
    """Logits of the net of L linears with the kernels' dropout masks of step gstep (None: no dropout)."""
    h = x.to(leaves[0].dtype)
    for l in range(L):
        skip, h = h, F.linear(h, leaves[2 * l], leaves[2 * l + 1])
        if l < L - 1:
            if norm == "layer":
                h = F.layer_norm(h, h.shape[-1:], leaves[2 * L + 2 * l], leaves[2 * L + 2 * l + 1], 1e-5)
            elif norm == "rms":
                h = leaves[2 * L + l] * h / torch.sqrt(h.pow(2).mean(-1, keepdim=True) + 1e-5)
            h = activation_fn(kind)(h)
            if gstep is not None:
                h = h * dropout_keep_mask(SEED, gstep, l, *h.shape, P_DROP).to(h.dtype) / (1 - P_DROP)
            h = skip + h if res and l == 1 else h
    return h


def _rel(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


def _check_grad(dims, B, loss, kind, norm, res, cuda, const_b0=None):
    flat, X, Y = _case(dims, B, norm, const_b0=const_b0)
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = _leaves(flat, dims, dt, norm)
        z = _forward(leaves, X, len(dims) - 1, kind, 0, norm, res)
        l = F.cross_entropy(z, Y) if loss == "ce" else F.mse_loss(z, F.one_hot(Y, z.shape[-1]).to(z.dtype))
        l.backward()
        ref[dt] = torch.cat([t.grad.reshape(-1) for t in leaves] + [l.detach().reshape(1)]).double()
    P, Pl = mlp_num_params(dims, norm), mlp_num_params(dims)
    g = torch.zeros(P + 1, device=cuda)
    FusedMLPKernel(dims, bmax=1024).train(
        flat.to(cuda), None, None, X.to(cuda), Y.to(cuda, torch.int32), torch.arange(B, dtype=torch.int32, device=cuda),
        n_items=B, batch=B, steps=1, t0=0, lr=0.01, dropout=P_DROP, seed=SEED, step_base=0, loss=loss, grad_out=g,
        activation=kind, norm=norm, residual=res)
    g, g64, g32 = g.cpu(), ref[torch.float64], ref[torch.float32]
    assert bool(torch.isfinite(g).all())
    # the whole gradient, the norm's words, the loss (whose fp32 reference can round to the fp64 one: floor 2^-24)
    groups = [(slice(0, P), 0.0), (slice(Pl, P), 0.0), (slice(P, P + 1), 2.0 ** -24)][:: 1 if norm else 2]
    errs = [(_rel(g[s], g64[s]), max(_rel(g32[s], g64[s]), floor)) for s, floor in groups]
    print("RES %s norm=%s res=%s %s B %d %s: (err, fp32 ref) of grad%s, loss:" % (
        kind, norm, res, dims, B, loss, ", norm words" if norm else ""), " ".join("(%.3e, %.3e)" % e for e in errs))
    assert all(e <= LIMIT * r for e, r in errs)


RES_SHAPES = [([5, 16, 16, 2], 17), ([7, 48, 48, 3], 40), ([32, 128, 128, 4], 33)]
RMS_SHAPES = [([5, 16, 2], 17), ([7, 48, 32, 3], 40)]


@pytest.mark.parametrize(
    "dims,B,loss,kind,norm,res,b0",
    [(d, B, "ce", kind, norm, True, None) for d, B in RES_SHAPES for norm in WORDS for kind in ("relu", "gelu")]
    + [([7, 48, 48, 3], 40, "mse", "relu", "rms", True, None)]
    + [(d, B, "ce", kind, "rms", False, None) for d, B in RMS_SHAPES for kind in ("relu", "gelu")]
    + [([5, 16, 2], 33, "ce", "relu", "rms", False, 0.0)])
def test_grad_mode_against_fp64(dims, B, loss, kind, norm, res, b0, cuda):
    """[5, 16, 16, 2] relu without a norm is the case a ReLU mask taken from A2 > 0 fails.  The last case: b0 = 0, so the
    pre-norm of the second tile's 31 dead rows is exactly 0, rstd = rsqrt(eps), and their zero gradient must stay zero."""
    _check_grad(dims, B, loss, kind, norm, res, cuda, const_b0=b0)


@pytest.mark.parametrize("composed", [False, True])
def test_train_mode_and_inference(composed, cuda):
    """Five Adam steps of residual + rms; composed: class weight, label smoothing, accumulate = 2 and clipping by norm."""
    dims, B, steps, kind, norm = [7, 48, 48, 3], 40, 5, "gelu", "rms"
    K = 2 if composed else 1
    cw = torch.tensor([0.5, 1.0, 2.0]) if composed else None
    flat, X, Y = _case(dims, 512, norm, seed=2)
    idx = torch.randperm(512, generator=torch.Generator().manual_seed(3))[: steps * K * B].to(torch.int32)
    leaves = _leaves(flat, dims, torch.float64, norm)
    opt = torch.optim.Adam(leaves, lr=0.01)
    ref_losses = []
    for s in range(steps):
        opt.zero_grad()
        for kb in range(s * K, s * K + K):
            rows = idx[kb * B:(kb + 1) * B].long()
            loss = F.cross_entropy(_forward(leaves, X[rows], 3, kind, kb, norm, True), Y[rows],
                                   weight=cw.double() if composed else None, label_smoothing=0.1 if composed else 0.0)
            (loss / K).backward()
        if composed:
            torch.nn.utils.clip_grad_norm_(leaves, 0.5)
        opt.step()
        ref_losses.append(float(loss.detach()))
    st = opt.state_dict()["state"]
    want, ref_m, ref_v = (torch.cat([t.detach().reshape(-1) for t in ts]) for ts in (
        leaves, [st[i]["exp_avg"] for i in range(len(st))], [st[i]["exp_avg_sq"] for i in range(len(st))]))

    k, p = FusedMLPKernel(dims, bmax=1024), flat.to(cuda)
    m, v, losses = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(steps, device=cuda)
    Xd, Yd = X.to(cuda), Y.to(cuda, torch.int32)
    opts = dict(class_weight=cw.to(cuda), label_smoothing=0.1, clip_val=0.5) if composed else {}
    k.train(p, m, v, Xd, Yd, idx.to(cuda), n_items=steps * K * B, batch=B, steps=steps, t0=0, lr=0.01, dropout=P_DROP,
            seed=SEED, step_base=0, loss_out=losses, activation=kind, norm=norm, residual=True, accumulate=K, **opts)
    err = (p.cpu().double() - want).abs()
    print("RES train composed=%s: param err median %.3e max %.3e" % (composed, err.median(), err.max()))
    # tests/test_tile_norm_gpu.py test_train_mode_and_inference's tolerances
    assert err.median() < 1e-5 and err.max() < 2e-3
    assert torch.allclose(losses.cpu().double(), torch.tensor(ref_losses, dtype=torch.float64), atol=2e-4, rtol=1e-3)
    assert torch.allclose(m.cpu().double(), ref_m, atol=1e-4, rtol=1e-2)
    assert torch.allclose(v.cpu().double(), ref_v, atol=1e-4, rtol=1e-2)
    # inference of the trained parameters over 100 rows with a repeated index
    ii = torch.arange(100, dtype=torch.int32) % 61
    logits = torch.zeros(100, dims[-1], device=cuda)
    k.infer(p, Xd, 100, idx=ii.to(cuda), logits_out=logits, activation=kind, hidden_norm=norm, residual=True)
    z64, z32 = (_forward(_leaves(p.cpu(), dims, dt, norm), X[ii.long()], 3, kind, None, norm, True).detach()
                for dt in (torch.float64, torch.float32))
    print("RES infer composed=%s: logits err %.3e (fp32 ref %.3e)" % (composed, _rel(logits.cpu(), z64), _rel(z32, z64)))
    assert _rel(logits.cpu(), z64) <= LIMIT * _rel(z32, z64)


@pytest.mark.parametrize("batch", [4, 64])
def test_engine_route(batch):
    """hidden=(64, 64), residual=True, norm="rms" under engine="auto": the fused engine on the tile plan, validation
    through the inference kernel, and norms.0.weight trained."""
    from torch.utils.data import DataLoader, random_split

    from dct_amd.data.dataset import TensorPairDataset
    from dct_amd.data.synthetic import weather_tensors
    from dct_amd.models.mlp import MLPClassifier
    from dct_amd.trainer import Trainer, seed_everything
    seed_everything(42)
    x, y = weather_tensors(6 * batch + 50, seed=0)
    tr, va = random_split(TensorPairDataset(x, y), [6 * batch, 50])
    model = MLPClassifier(5, hidden=(64, 64), residual=True, norm="rms")
    t = Trainer(max_epochs=1, accelerator="gpu", engine="auto", logger=None, num_sanity_val_steps=0, verbose=False)
    t.fit(model, DataLoader(tr, batch_size=batch, shuffle=True), DataLoader(va, batch_size=32))
    assert t.engine.name == "fused" and t.engine.kernel.plan.trainer(batch, norm="rms", residual=True) == "tile"
    (got,) = t.validate(model, DataLoader(va, batch_size=32))  # (syncs the engine's flat parameters into the module)
    with torch.no_grad():
        z = model.cpu().eval()(x[va.indices])
    assert abs(got["val_loss"] - float(F.cross_entropy(z, y[va.indices]))) <= 1e-5
    assert "norms.0.bias" not in model.state_dict() and float((model.norms[0].weight - 1).abs().min()) > 0
