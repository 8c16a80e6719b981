"""LayerNorm hidden layers in the batch-tiled MLP trainer and inference kernel (csrc/mlp_tile.hip, csrc/mlp_infer.hip)
on the GPU, against the same net in torch fp64 autograd on the CPU under the host dropout masks.

The measure, as in test_tile_act_gpu.py: max|x - x64| / max|x64|, held to LIMIT times the same quantity of torch's own
fp32 CPU autograd on the same case; the LayerNorm words (dgamma, dbeta) also as a group of their own, so a wrong tail
cannot hide under the larger W1 words.  LIMIT follows that file's rule - 4 x the largest measured ratio, capped at 32,
and 8 where the ratios fit under it; the measured ratios are in profiles/tile_norm_cost.log."""
import pytest
import torch
import torch.nn.functional as F

from dct_amd.ops.fused_mlp import FusedMLPKernel, activation_fn, dropout_keep_mask, mlp_num_params

pytestmark = pytest.mark.gpu

LIMIT = 8.0
P_DROP, SEED = 0.2, 11


def _case(dims, n, seed=1, const_b0=None):
    """Flat parameters in the kernels' order - all linears, then gamma_l, beta_l of the hidden layers - and data."""
    g = torch.Generator().manual_seed(seed)
    parts = [t for i, o in zip(dims[:-1], dims[1:])
             for t in (torch.randn(o * i, generator=g) / i ** 0.5, torch.randn(o, generator=g) * 0.1)]
    if const_b0 is not None:
        parts[1] = torch.full_like(parts[1], const_b0)
    for h in dims[1:-1]:
        parts += [0.5 + torch.rand(h, generator=g), torch.randn(h, generator=g) * 0.1]
    X = torch.randn(n, dims[0], generator=g)
    Y = torch.randint(0, dims[-1], (n,), generator=g)
    return torch.cat(parts), X, Y


def _leaves(flat, dims, dt):
    shapes = [s for i, o in zip(dims[:-1], dims[1:]) for s in ((o, i), (o,))] + [(h,) for h in dims[1:-1] for _ in "gb"]
    leaves, off = [], 0
    for s in shapes:
        n = s[0] * (s[1] if len(s) == 2 else 1)
        leaves.append(flat[off: off + n].view(s).to(dt).requires_grad_())
        off += n
    return leaves


def _forward(leaves, x, kind, gstep):
    """Logits of the net with the kernels' dropout masks of step gstep (None: no dropout)."""
    L = (len(leaves) + 2) // 4
    h = x.to(leaves[0].dtype)
    for l in range(L):
        h = F.linear(h, leaves[2 * l], leaves[2 * l + 1])
        if l < L - 1:
            h = F.layer_norm(h, h.shape[-1:], leaves[2 * L + 2 * l], leaves[2 * L + 2 * l + 1], 1e-5)
            h = activation_fn(kind)(h)
            if gstep is not None:
                h = h * dropout_keep_mask(SEED, gstep, l, *h.shape, P_DROP).to(h.dtype) / (1 - P_DROP)
    return h


def _rel(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


def _check_grad(dims, B, loss, kind, cuda, const_b0=None):
    flat, X, Y = _case(dims, B, const_b0=const_b0)
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = _leaves(flat, dims, dt)
        z = _forward(leaves, X, kind, 0)
        l = F.cross_entropy(z, Y) if loss == "ce" else F.mse_loss(z, F.one_hot(Y, z.shape[-1]).to(z.dtype))
        l.backward()
        ref[dt] = (torch.cat([t.grad.reshape(-1) for t in leaves]).double(), l.detach().double())
    P, Pl = mlp_num_params(dims, "layer"), mlp_num_params(dims)
    g = torch.zeros(P + 1, device=cuda)
    FusedMLPKernel(dims, bmax=1024).train(
        flat.to(cuda), None, None, X.to(cuda), Y.to(cuda, torch.int32), torch.arange(B, dtype=torch.int32, device=cuda),
        n_items=B, batch=B, steps=1, t0=0, lr=0.01, dropout=P_DROP, seed=SEED, step_base=0, loss=loss, grad_out=g,
        activation=kind, norm="layer")
    g = g.cpu()
    assert bool(torch.isfinite(g).all())
    (g64, l64), g32 = ref[torch.float64], ref[torch.float32][0]
    eg, rg = _rel(g[:P], g64), _rel(g32, g64)
    en, rn = _rel(g[Pl:P], g64[Pl:]), _rel(g32[Pl:], g64[Pl:])
    el, rl = abs(float(g[P]) - float(l64)) / abs(float(l64)), abs(float(ref[torch.float32][1] - l64)) / abs(float(l64))
    print("NORM %s %s B %d %s: grad err %.3e (fp32 ref %.3e, ratio %.2f) norm words %.3e (%.3e, ratio %.2f) "
          "loss err %.3e (fp32 ref %.3e)" % (kind, dims, B, loss, eg, rg, eg / rg, en, rn, en / rn, el, rl))
    assert eg <= LIMIT * rg and en <= LIMIT * rn
    assert el <= LIMIT * max(rl, 2.0 ** -24)  # (the fp32 reference's loss can round to the fp64 one exactly)


SHAPES = [([5, 16, 2], 17), ([7, 48, 32, 3], 40), ([32, 128, 128, 4], 33)]


@pytest.mark.parametrize("dims,B,loss,kind", [(d, B, "ce", kind) for d, B in SHAPES for kind in ("relu", "gelu")]
                         + [([7, 48, 32, 3], 40, "mse", "relu")])
def test_grad_mode_against_fp64(dims, B, loss, kind, cuda):
    _check_grad(dims, B, loss, kind, cuda)


def test_dead_rows_of_zero_variance(cuda):
    """B = 33 with all of b0 equal: the 31 dead rows of the second tile have variance 0, rstd = rsqrt(eps) - and their
    zero gradient must stay a zero, not 0 * inf."""
    _check_grad([5, 16, 2], 33, "ce", "relu", cuda, const_b0=0.3)


@pytest.mark.parametrize("composed", [False, True])
def test_train_mode_and_inference(composed, cuda):
    """Five Adam steps; composed: with a class weight, label smoothing, accumulate = 2 and clipping by norm."""
    dims, B, steps, n_inf, kind = [7, 48, 32, 3], 40, 5, 100, "gelu"
    K = 2 if composed else 1
    cw = torch.tensor([0.5, 1.0, 2.0]) if composed else None
    opts = dict(class_weight=cw, label_smoothing=0.1, clip_val=0.5) if composed else {}
    flat, X, Y = _case(dims, 512, seed=2)
    idx = torch.randperm(512, generator=torch.Generator().manual_seed(3))[: steps * K * B].to(torch.int32)
    leaves = _leaves(flat, dims, torch.float64)
    opt = torch.optim.Adam(leaves, lr=0.01)
    ref_losses = []
    for s in range(steps):
        opt.zero_grad()
        for kb in range(K):
            rows = idx[(s * K + kb) * B:(s * K + kb + 1) * B].long()
            z = _forward(leaves, X[rows], kind, s * K + kb)
            loss = (F.cross_entropy(z, Y[rows], weight=cw.double(), label_smoothing=0.1) if composed
                    else F.cross_entropy(z, Y[rows]))
            (loss / K).backward()
        if composed:
            torch.nn.utils.clip_grad_norm_(leaves, 0.5)
        opt.step()
        ref_losses.append(float(loss))
    want = torch.cat([t.detach().reshape(-1) for t in leaves])
    st = opt.state_dict()["state"]
    ref_m = torch.cat([st[i]["exp_avg"].reshape(-1) for i in range(len(st))])
    ref_v = torch.cat([st[i]["exp_avg_sq"].reshape(-1) for i in range(len(st))])

    k = FusedMLPKernel(dims, bmax=1024)
    p = flat.to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(steps, device=cuda)
    Xd, Yd = X.to(cuda), Y.to(cuda, torch.int32)
    opts.update(class_weight=cw.to(cuda)) if composed else None
    k.train(p, m, v, Xd, Yd, idx.to(cuda), n_items=steps * K * B, batch=B, steps=steps, t0=0, lr=0.01, dropout=P_DROP,
            seed=SEED, step_base=0, loss_out=losses, activation=kind, norm="layer", accumulate=K, **opts)
    err = (p.cpu().double() - want).abs()
    print("NORM train composed=%s: param err median %.3e max %.3e (norm words max %.3e)"
          % (composed, err.median(), err.max(), err[mlp_num_params(dims):].max()))
    # tests/test_tile_act_gpu.py test_train_mode_and_inference's tolerances
    assert err.median() < 1e-5 and err.max() < 2e-3
    assert torch.allclose(losses.cpu().double(), torch.tensor(ref_losses, dtype=torch.float64), atol=2e-4, rtol=1e-3)
    assert torch.allclose(m.cpu().double(), ref_m, atol=1e-4, rtol=1e-2)
    assert torch.allclose(v.cpu().double(), ref_v, atol=1e-4, rtol=1e-2)

    # inference of the trained parameters over 100 rows with a repeated index
    ii = torch.arange(n_inf, dtype=torch.int32) % 61
    logits = torch.zeros(n_inf, dims[-1], device=cuda)
    k.infer(p, Xd, n_inf, idx=ii.to(cuda), logits_out=logits, activation=kind, hidden_norm="layer")
    z64, z32 = (_forward(_leaves(p.cpu(), dims, dt), X[ii.long()], kind, None).detach()
                for dt in (torch.float64, torch.float32))
    ez, rz = _rel(logits.cpu(), z64), _rel(z32, z64)
    print("NORM infer composed=%s: logits err %.3e (fp32 ref %.3e, ratio %.2f)" % (composed, ez, rz, ez / rz))
    assert ez <= LIMIT * rz


@pytest.mark.parametrize("batch", [4, 64])
def test_engine_route(batch):
    """A normed WeatherClassifier under engine="auto": the fused engine on the tile plan, validation through the
    inference kernel, and norms.0.* trained."""
    from torch.utils.data import DataLoader, random_split

    from dct_amd.data.dataset import TensorPairDataset
    from dct_amd.data.synthetic import weather_tensors
    from dct_amd.models.mlp import WeatherClassifier
    from dct_amd.trainer import Trainer, seed_everything
    seed_everything(42)
    x, y = weather_tensors(6 * batch + 50, seed=0)
    tr, va = random_split(TensorPairDataset(x, y), [6 * batch, 50])
    model = WeatherClassifier(5, norm="layer")
    t = Trainer(max_epochs=1, accelerator="gpu", engine="auto", logger=None, num_sanity_val_steps=0, verbose=False)
    val = DataLoader(va, batch_size=32)
    t.fit(model, DataLoader(tr, batch_size=batch, shuffle=True), val)
    eng = t.engine
    assert eng.name == "fused" and eng.kernel.plan.trainer(batch, norm="layer") == "tile"
    ref = WeatherClassifier(5, norm="layer").eval()
    with torch.no_grad():
        torch.nn.utils.vector_to_parameters(eng.p.cpu(), ref.parameters())  # (flat order = parameters() order)
        xv, yv = x[va.indices], y[va.indices]
        z = ref(xv)
    want_loss, want_acc = float(F.cross_entropy(z, yv)), int((z.argmax(1) == yv).sum()) / len(yv)
    got = t.callback_metrics
    assert abs(float(got["val_loss"]) - want_loss) <= 1e-5 and float(got["val_acc"]) == want_acc
    (again,) = t.validate(model, val)
    assert abs(again["val_loss"] - want_loss) <= 1e-5 and again["val_acc"] == want_acc
    sd = model.state_dict()  # (validate synced the engine's flat parameters into the module)
    assert torch.equal(sd["norms.0.weight"].cpu(), ref.norms[0].weight) and torch.equal(sd["net.3.bias"].cpu(), ref.net[3].bias)
    assert float((sd["norms.0.weight"] - 1).abs().min()) > 0 and float(sd["norms.0.bias"].abs().min()) > 0
