"""GELU / tanh-GELU / SiLU in the batch-tiled MLP trainer and inference kernel (csrc/mlp_tile.hip, csrc/mlp_infer.hip)
on the GPU, against the same net in torch fp64 autograd on the CPU under the host dropout masks.

The measure of tests 1 and 2: max|x - x64| / max|x64|, held to LIMIT times the same quantity of torch's own fp32 CPU
autograd on the same case.  Measured on an MI355X (profiles/tile_act_cost.log): the kernel / fp32-reference ratio of the
gradient is 0.52 .. 2.00 over the twelve cases (worst: silu, [7, 48, 32, 3] MSE), of the logits 0.88 .. 1.67, so
LIMIT = 4 * 2.00 = 8 (the cap is 32).  A scalar loss has no max over many words to steady its reference error - the
fp32 reference's loss can land within 1e-9 of the fp64 one - so there the reference error counts as at least
2^-24, the half ulp of rounding the fp64 loss to fp32.  The nearest wrong kernel, erf-GELU for tanh-GELU, is off by a
ratio >= 680."""
import pytest
import torch
import torch.nn.functional as F

from dct_amd.ops.fused_mlp import FusedMLPKernel, activation_fn, dropout_keep_mask, mlp_num_params

pytestmark = pytest.mark.gpu

KINDS = ["gelu", "gelu_tanh", "silu"]
LIMIT = 8.0
P_DROP, SEED = 0.2, 11


def _case(dims, n, seed=1):
    g = torch.Generator().manual_seed(seed)
    flat = torch.cat([t for i, o in zip(dims[:-1], dims[1:])
                      for t in (torch.randn(o * i, generator=g) / i ** 0.5, torch.randn(o, generator=g) * 0.1)])
    X = torch.randn(n, dims[0], generator=g)
    Y = torch.randint(0, dims[-1], (n,), generator=g)
    return flat, X, Y


def _leaves(flat, dims, dt):
    leaves, off = [], 0
    for i, o in zip(dims[:-1], dims[1:]):
        leaves += [flat[off: off + i * o].view(o, i).to(dt).requires_grad_(),
                   flat[off + i * o: off + i * o + o].to(dt).requires_grad_()]
        off += i * o + o
    return leaves


def _forward(leaves, x, kind, gstep):
    """Logits of the net with the kernels' dropout masks of step gstep (None: no dropout)."""
    h, L = x.to(leaves[0].dtype), len(leaves) // 2
    for l in range(L):
        h = F.linear(h, leaves[2 * l], leaves[2 * l + 1])
        if l < L - 1:
            h = activation_fn(kind)(h)
            if gstep is not None:
                h = h * dropout_keep_mask(SEED, gstep, l, *h.shape, P_DROP).to(h.dtype) / (1 - P_DROP)
    return h


def _loss(z, y, loss):
    return F.cross_entropy(z, y) if loss == "ce" else F.mse_loss(z, F.one_hot(y, z.shape[-1]).to(z.dtype))


def _rel(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims,B,loss", [([5, 64, 2], 17, "ce"), ([7, 48, 32, 3], 40, "ce"), ([7, 48, 32, 3], 40, "mse"),
                                         ([32, 128, 128, 4], 33, "ce")])
def test_grad_mode_against_fp64(dims, B, loss, kind, cuda):
    flat, X, Y = _case(dims, B)
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = _leaves(flat, dims, dt)
        l = _loss(_forward(leaves, X, kind, 0), Y, loss)
        l.backward()
        ref[dt] = (torch.cat([t.grad.reshape(-1) for t in leaves]).double(), l.detach().double())
    P = mlp_num_params(dims)
    g = torch.zeros(P + 1, device=cuda)
    FusedMLPKernel(dims, bmax=1024).train(
        flat.to(cuda), None, None, X.to(cuda), Y.to(cuda, torch.int32), torch.arange(B, dtype=torch.int32, device=cuda),
        n_items=B, batch=B, steps=1, t0=0, lr=0.01, dropout=P_DROP, seed=SEED, step_base=0, loss=loss, grad_out=g,
        activation=kind)
    g = g.cpu()
    g64, l64 = ref[torch.float64]
    eg, el = _rel(g[:P], g64), abs(float(g[P]) - float(l64)) / abs(float(l64))
    rg, rl = _rel(ref[torch.float32][0], g64), abs(float(ref[torch.float32][1] - l64)) / abs(float(l64))
    print("ACT %s %s B %d %s: grad err %.3e (fp32 ref %.3e, ratio %.2f) loss err %.3e (fp32 ref %.3e)"
          % (kind, dims, B, loss, eg, rg, eg / rg, el, rl))
    assert eg <= LIMIT * rg
    assert el <= LIMIT * max(rl, 2.0 ** -24)  # (the fp32 reference's loss can round to the fp64 one exactly)


@pytest.mark.parametrize("kind", KINDS)
def test_train_mode_and_inference(kind, cuda):
    dims, B, steps, n_inf = [7, 48, 32, 3], 40, 3, 100
    flat, X, Y = _case(dims, 128, seed=2)
    idx = torch.randperm(128, generator=torch.Generator().manual_seed(3))[: steps * B].to(torch.int32)
    # torch fp64 Adam under the same masks
    leaves = _leaves(flat, dims, torch.float64)
    opt = torch.optim.Adam(leaves, lr=0.01)
    ref_losses = []
    for s in range(steps):
        rows = idx[s * B:(s + 1) * B].long()
        opt.zero_grad()
        loss = F.cross_entropy(_forward(leaves, X[rows], kind, s), Y[rows])
        loss.backward()
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
    k.train(p, m, v, Xd, Yd, idx.to(cuda), n_items=steps * B, batch=B, steps=steps, t0=0, lr=0.01, dropout=P_DROP,
            seed=SEED, step_base=0, loss_out=losses, activation=kind)
    err = (p.cpu().double() - want).abs()
    print("ACT %s train: param err median %.3e max %.3e" % (kind, err.median(), err.max()))
    # tests/test_mlp_tile_gpu.py _check_against_torch's tolerances
    assert err.median() < 1e-5 and err.max() < 2e-3
    assert torch.allclose(losses.cpu().double(), torch.tensor(ref_losses, dtype=torch.float64), atol=2e-4, rtol=1e-3)
    assert torch.allclose(m.cpu().double(), ref_m, atol=1e-4, rtol=1e-2)
    assert torch.allclose(v.cpu().double(), ref_v, atol=1e-4, rtol=1e-2)

    # inference of the trained parameters over 100 rows with a repeated index
    ii = torch.arange(n_inf, dtype=torch.int32) % 61
    logits = torch.zeros(n_inf, dims[-1], device=cuda)
    stats = torch.zeros(2 + dims[-1] ** 2, dtype=torch.int64, device=cuda)
    k.infer(p, Xd, n_inf, idx=ii.to(cuda), Y=Yd, logits_out=logits, stats_out=stats, activation=kind)
    loss_sum, correct, conf = k.infer_stats(stats)
    z64, z32 = (_forward(_leaves(p.cpu(), dims, dt), X[ii.long()], kind, None).detach()
                for dt in (torch.float64, torch.float32))
    y = Y[ii.long()]
    ez, rz = _rel(logits.cpu(), z64), _rel(z32, z64)
    print("ACT %s infer: logits err %.3e (fp32 ref %.3e, ratio %.2f)" % (kind, ez, rz, ez / rz))
    assert ez <= LIMIT * rz
    l64 = float(F.cross_entropy(z64, y, reduction="sum"))
    # a row's fp32 loss mx + log(se) - z_y: three terms below 8 (half an ulp each, 2.4e-7) on logits good to 1e-6
    assert abs(loss_sum - l64) <= n_inf * 4e-6
    pred = z64.argmax(1)
    assert correct == int((pred == y).sum())
    assert torch.equal(conf, torch.bincount(y * dims[-1] + pred, minlength=dims[-1] ** 2).reshape(dims[-1], dims[-1]))


def test_engine_route():
    """A SiLU model under engine="auto": the fused engine on the tile plan, validation through the inference kernel."""
    from torch.utils.data import DataLoader, random_split

    from dct_amd.data.dataset import TensorPairDataset
    from dct_amd.data.synthetic import weather_tensors
    from dct_amd.models.mlp import MLPClassifier
    from dct_amd.trainer import Trainer, seed_everything

    seed_everything(42)
    x, y = weather_tensors(6 * 32 + 50, seed=0)
    tr, va = random_split(TensorPairDataset(x, y), [6 * 32, 50])
    model = MLPClassifier(5, hidden=(64,), activation="silu")
    t = Trainer(max_epochs=1, accelerator="gpu", engine="auto", logger=None, num_sanity_val_steps=0, verbose=False)
    val = DataLoader(va, batch_size=32)
    t.fit(model, DataLoader(tr, batch_size=32, shuffle=True), val)
    eng = t.engine
    assert eng.name == "fused" and eng.kernel.plan.trainer(32, activation="silu") == "tile"
    ref = MLPClassifier(5, hidden=(64,), activation="silu").eval()
    with torch.no_grad():
        torch.nn.utils.vector_to_parameters(eng.p.cpu(), ref.parameters())  # (state_dict order = parameter order)
        xv, yv = x[va.indices], y[va.indices]
        z = ref(xv)
    want_loss, want_acc = float(F.cross_entropy(z, yv)), int((z.argmax(1) == yv).sum()) / len(yv)
    got = t.callback_metrics
    assert abs(float(got["val_loss"]) - want_loss) <= 1e-5 and float(got["val_acc"]) == want_acc
    (again,) = t.validate(model, val)
    assert abs(again["val_loss"] - want_loss) <= 1e-5 and again["val_acc"] == want_acc
