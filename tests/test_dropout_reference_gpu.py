"""Dropout-on steps of every fused trainer against a float64 reference under the host mirrors' masks
(run on a real MI355X).

The reference is a float64 torch net with the kernel's weights whose forward is
``relu(lin(h)) * keep * (1 / (1 - p))`` with ``keep`` from ``FusedMLPKernel.dropout_mask`` (the wave
kernels' hash or the mix_hash family, by the launcher's own rule); gradients come from autograd.  Every
problem is built from the first of 8 fixed seeds whose reference has no hidden pre-activation within
1e-5 of the ReLU boundary on a live row, so a kernel's fp32 rounding cannot flip a unit.

Kernels per case: WAVE_GRAD -> single-wave kernel (grad mode), LDS_GRAD -> generic LDS trainer,
BLOCK3_GRAD -> mlp_block3, BLOCK5_GRAD -> mlp_block5 / mlp_block5_b8 (batch 5..8), TILE_GRAD -> mlp_tile,
ROWS_TRAIN -> wave_rows_x0 (train mode), OTHER_TRAIN -> the train-mode instantiations of the rest."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dct_amd  # noqa: F401
from dct_amd.ops._native import native
from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params
from test_mlp_tile_gpu import _check_against_torch  # the project's trajectory bounds, shared

pytestmark = pytest.mark.gpu

PDROP, SEED, STEP_BASE, LR = 0.2, 0x5EED1234, 5, 0.01
PROBLEM_SEEDS = range(40, 48)
RELU_MARGIN = 1e-5
GRAD_ATOL, GRAD_RTOL, LOSS_TOL = 1e-6, 1e-4, 1e-5  # test_fused_grad_mode_matches_autograd's
# the kernels get fp32 hyper-parameters: the reference uses the same numbers, exactly
P32 = float(np.float32(PDROP))
ONE_MINUS_B1 = float(np.float32(1) - np.float32(0.9))
ONE_MINUS_B2 = float(np.float32(1) - np.float32(0.999))

NO_ENV, LDS, BLOCK0, BLOCK3 = {}, {"DCT_MLP_KERNEL": "lds"}, {"DCT_MLP_BLOCK": "0"}, {"DCT_MLP_BLOCK": "3"}


@pytest.fixture(autouse=True)
def _fresh_knobs():
    """The native launchers read their DCT_* knobs at plan / bind time: every test starts from (and
    leaves) the environment as it is outside the test's monkeypatch."""
    native().reload_knobs()
    yield
    native().reload_knobs()


def _kernel(dims, B, env, monkeypatch):
    for name in ("DCT_MLP_KERNEL", "DCT_MLP_BLOCK"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    k = FusedMLPKernel(dims, bmax=4 if B <= 4 else (16 if B <= 16 else 1024))  # the plan re-reads the knobs
    assert k.plan.supported
    return k


def _ref_net(dims):
    layers = []
    for i in range(len(dims) - 1):
        layers.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(torch.nn.ReLU())
    return torch.nn.Sequential(*layers)


def _flat(net):
    return torch.cat([t.detach().reshape(-1) for t in net.state_dict().values()])


def _flat_grad(net):
    return torch.cat([q.grad.reshape(-1) for q in net.parameters()])


class _Reference:
    """The float64 net under the host mirror's masks; records the smallest hidden |pre-activation|."""

    def __init__(self, net32, k, B):
        self.net = copy.deepcopy(net32).double()
        self.B = B  # the launch's batch: the hash family and the keys do not depend on how many rows are live
        self.lins = [l for l in self.net if isinstance(l, torch.nn.Linear)]
        self.k = k
        self.min_abs_z = math.inf

    def loss(self, x, y, gstep, kind):
        h = x.double()
        for li, lin in enumerate(self.lins[:-1]):
            z = lin(h)
            self.min_abs_z = min(self.min_abs_z, float(z.detach().abs().min()))
            keep = self.k.dropout_mask(SEED, gstep, li, self.B, PDROP)[:x.shape[0]]
            h = torch.relu(z) * keep * (1.0 / (1.0 - P32))
        logits = self.lins[-1](h)
        if kind == "ce":
            return F.cross_entropy(logits, y)
        return F.mse_loss(logits, F.one_hot(y, logits.shape[1]).double())


def _build(dims, B, n_items, k, run_ref):
    """The problem of the first seed whose reference run ``run_ref(ref, X, Y, idx)`` stays off the ReLU
    boundary: (X, Y, idx, initial fp32 net, reference, what run_ref returned)."""
    for s in PROBLEM_SEEDS:
        torch.manual_seed(s)
        N = n_items + 37
        X = torch.randn(N, dims[0])
        Y = torch.randint(0, dims[-1], (N,))
        idx = torch.randperm(N)[:n_items]
        net = _ref_net(dims)
        ref = _Reference(net, k, B)
        out = run_ref(ref, X, Y, idx)
        if ref.min_abs_z >= RELU_MARGIN:
            print("problem seed %d, min |z| %.3e" % (s, ref.min_abs_z))
            return X, Y, idx, net, ref, out
    pytest.fail("no problem seed in %r keeps the reference off the ReLU boundary" % (PROBLEM_SEEDS,))


def _excess(got, want, atol, rtol):
    """Worst excess of |got - want| over atol + rtol |want| (torch.allclose's bound); <= 0 passes."""
    want = want.double()
    err, tol = (got.double().cpu() - want).abs(), atol + rtol * want.abs()
    print("  worst error / tolerance %.4f" % float((err / tol).max()))
    return float((err - tol).max())


def _one_step_reference(n_items, loss):
    def run(ref, X, Y, idx):
        rows = idx[:n_items]
        l = ref.loss(X[rows], Y[rows], STEP_BASE, loss)
        l.backward()
        return _flat_grad(ref.net), float(l.detach())
    return run


def _dead_row_sibling(B):
    return B - 1 if B <= 4 else B - B // 3


def _with_siblings(cases):
    """(dims, B, env) -> (dims, B, n_items, env): the full batch and, where the batch has a row to lose,
    a partial one (dead rows; whole empty tiles in the batch-tiled trainer)."""
    out = []
    for dims, B, env in cases:
        out.append((dims, B, B, env))
        if B > 1:
            out.append((dims, B, _dead_row_sibling(B), env))
    return out


# ------------------------------------------------------------------ a. grad mode, one launch
WAVE_GRAD = [([5, 64, 2], 4, NO_ENV), ([5, 64, 2], 3, NO_ENV), ([7, 20, 2], 8, NO_ENV), ([16, 64, 4], 5, NO_ENV),
             ([9, 48, 64, 3], 4, NO_ENV), ([9, 48, 64, 3], 8, NO_ENV), ([12, 40, 40, 4], 6, NO_ENV)]
LDS_GRAD = [([5, 64, 2], 16, NO_ENV), ([7, 20, 2], 9, NO_ENV), ([12, 40, 4], 6, LDS), ([16, 32, 48, 32, 3], 16, NO_ENV),
            ([5, 128, 128, 2], 4, BLOCK0)]
BLOCK3_GRAD = [([7, 128, 128, 2], 4, BLOCK3), ([30, 128, 128, 3], 3, BLOCK3)]
BLOCK5_GRAD = [([5, 128, 128, 2], 4, NO_ENV, "block5"), ([5, 128, 128, 2], 3, NO_ENV, "block5"),
               ([8, 128, 128, 2], 1, NO_ENV, "block5"), ([1, 128, 128, 2], 2, NO_ENV, "block5"),
               ([5, 128, 128, 2], 8, NO_ENV, "block5_b8"), ([3, 128, 128, 2], 7, NO_ENV, "block5_b8")]
TILE_GRAD = [([5, 64, 2], 17, NO_ENV), ([5, 128, 128, 2], 33, NO_ENV), ([5, 128, 128, 2], 100, NO_ENV),
             ([7, 48, 32, 3], 65, NO_ENV), ([7, 32, 48, 3], 40, NO_ENV), ([32, 128, 128, 4], 17, NO_ENV)]


def _check_plan(k, B, trainer, mode):
    """The plan names the trainer this case's launch reaches (csrc/mlp_select.h): the kernel under test."""
    assert k.plan.trainer(B, mode=mode) == trainer


FAMILY = {"wave_single": "wave", "wave_rows": "wave", "block5": "block", "block5_b8": "block", "block3": "block",
          "lds": "lds", "tile": "tile"}


def _ids(params, family=False):
    """Ids of (dims, B, [n_items,] env, trainer) cases: those they had before they named their trainer (with
    ``family``, when they named a kernel family), so a case's history stays under one id."""
    return ["-".join(["dims%d" % i] + [str(x) for x in p[1:-2]] + ["env%d" % i] + ([FAMILY[p[-1]]] if family else []))
            for i, p in enumerate(params)]


def _grad_case(dims, B, n_items, env, loss, trainer, cuda, monkeypatch):
    k = _kernel(dims, B, env, monkeypatch)
    _check_plan(k, B, trainer, mode=1)
    X, Y, idx, net, _, (want, want_loss) = _build(dims, B, n_items, k, _one_step_reference(n_items, loss))
    P = mlp_num_params(dims)
    p = _flat(net).to(cuda)
    g = torch.zeros(P + 1, device=cuda)
    k.train(p, None, None, X.to(cuda), Y.to(cuda, torch.int32), idx.to(cuda, torch.int32), n_items=n_items, batch=B,
            steps=1, t0=0, lr=LR, dropout=PDROP, seed=SEED, step_base=STEP_BASE, loss=loss, grad_out=g)
    torch.cuda.synchronize()
    ex = _excess(g[:P], want, GRAD_ATOL, GRAD_RTOL)
    lerr = abs(g[P].item() - want_loss)
    print("grad excess over tolerance %.3e (max |g| %.3e), loss err %.3e of %.0e" % (ex, want.abs().max(), lerr, LOSS_TOL))
    assert torch.isfinite(g).all()
    assert ex <= 0, ex
    assert lerr < LOSS_TOL, lerr


BLOCK5_GRAD_CASES = [c + (t,) for d, b, e, t in BLOCK5_GRAD for c in _with_siblings([(d, b, e)])]


@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dims,B,n_items,env", _with_siblings(WAVE_GRAD))
def test_wave_grad_mode_matches_fp64_under_host_mask(dims, B, n_items, env, loss, cuda, monkeypatch):
    _grad_case(dims, B, n_items, env, loss, "wave_single", cuda, monkeypatch)


@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dims,B,n_items,env", _with_siblings(LDS_GRAD))
def test_lds_grad_mode_matches_fp64_under_host_mask(dims, B, n_items, env, loss, cuda, monkeypatch):
    _grad_case(dims, B, n_items, env, loss, "lds", cuda, monkeypatch)


@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dims,B,n_items,env", _with_siblings(BLOCK3_GRAD))
def test_block3_grad_mode_matches_fp64_under_host_mask(dims, B, n_items, env, loss, cuda, monkeypatch):
    _grad_case(dims, B, n_items, env, loss, "block3", cuda, monkeypatch)


@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dims,B,n_items,env,trainer", BLOCK5_GRAD_CASES, ids=_ids(BLOCK5_GRAD_CASES))
def test_block5_grad_mode_matches_fp64_under_host_mask(dims, B, n_items, env, trainer, loss, cuda, monkeypatch):
    _grad_case(dims, B, n_items, env, loss, trainer, cuda, monkeypatch)


@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dims,B,n_items,env", _with_siblings(TILE_GRAD))
def test_tile_grad_mode_matches_fp64_under_host_mask(dims, B, n_items, env, loss, cuda, monkeypatch):
    _grad_case(dims, B, n_items, env, loss, "tile", cuda, monkeypatch)


# ------------------------------------------------------------------ b. train mode, one step from zero moments
ROWS_TRAIN = [([5, 64, 2], 4, NO_ENV), ([5, 64, 2], 8, NO_ENV), ([5, 64, 2], 3, NO_ENV), ([8, 48, 3], 5, NO_ENV),
              ([16, 64, 4], 2, NO_ENV)]
OTHER_TRAIN = [([5, 128, 128, 2], 4, NO_ENV, "block5"), ([5, 128, 128, 2], 8, NO_ENV, "block5_b8"),
               ([5, 128, 128, 2], 4, BLOCK3, "block3"), ([5, 64, 2], 16, NO_ENV, "lds"),
               ([5, 128, 128, 2], 33, NO_ENV, "tile")]
OTHER_TRAIN_CASES = [c + (t,) for d, b, e, t in OTHER_TRAIN for c in _with_siblings([(d, b, e)])]


def _train_step_case(dims, B, n_items, env, loss, trainer, cuda, monkeypatch):
    """After one Adam step from m = v = 0 without weight decay, m / (1 - beta1) is the gradient and
    sqrt(v / (1 - beta2)) its magnitude."""
    k = _kernel(dims, B, env, monkeypatch)
    _check_plan(k, B, trainer, mode=0)
    X, Y, idx, net, _, (want, want_loss) = _build(dims, B, n_items, k, _one_step_reference(n_items, loss))
    p = _flat(net).to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(1, device=cuda)
    k.train(p, m, v, X.to(cuda), Y.to(cuda, torch.int32), idx.to(cuda, torch.int32), n_items=n_items, batch=B,
            steps=1, t0=0, lr=LR, weight_decay=0.0, dropout=PDROP, seed=SEED, step_base=STEP_BASE, loss=loss,
            loss_out=losses)
    torch.cuda.synchronize()
    ex_m = _excess(m.double() / ONE_MINUS_B1, want, GRAD_ATOL, GRAD_RTOL)
    ex_v = _excess((v.double() / ONE_MINUS_B2).sqrt(), want.abs(), GRAD_ATOL, GRAD_RTOL)
    lerr = abs(losses.item() - want_loss)
    print("m excess over tolerance %.3e, sqrt(v) excess %.3e (max |g| %.3e), loss err %.3e of %.0e"
          % (ex_m, ex_v, want.abs().max(), lerr, LOSS_TOL))
    assert torch.isfinite(p).all() and torch.isfinite(m).all() and torch.isfinite(v).all()
    assert ex_m <= 0, ex_m
    assert ex_v <= 0, ex_v
    assert lerr < LOSS_TOL, lerr
    # the step moved the parameters against the gradient's sign wherever the gradient is not tiny
    moved = (p.cpu().double() - _flat(net).double())
    big = want.abs() > 1e-4
    assert bool((torch.sign(moved[big]) == -torch.sign(want[big])).all())


@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dims,B,n_items,env", _with_siblings(ROWS_TRAIN))
def test_rows_kernel_train_step_matches_fp64_under_host_mask(dims, B, n_items, env, loss, cuda, monkeypatch):
    assert len(dims) == 3 and B <= 8  # wave_rows_x0's launches (csrc/mlp_wave.hip mlp_wave_rows_takes)
    _train_step_case(dims, B, n_items, env, loss, "wave_rows", cuda, monkeypatch)


@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dims,B,n_items,env,trainer", OTHER_TRAIN_CASES, ids=_ids(OTHER_TRAIN_CASES, family=True))
def test_train_step_matches_fp64_under_host_mask(dims, B, n_items, env, trainer, loss, cuda, monkeypatch):
    _train_step_case(dims, B, n_items, env, loss, trainer, cuda, monkeypatch)


# ------------------------------------------------------------------ c. trajectories
STEPS = 7


def _adam_reference(B, n_items, first_gstep, loss):
    """fp64 torch.optim.Adam over the index list; step s draws the mirror's mask of step first_gstep + s
    and is Adam step first_gstep + s + 1 (zero moments at the start)."""
    def run(ref, X, Y, idx):
        opt = torch.optim.Adam(ref.net.parameters(), lr=LR)
        for q in ref.net.parameters():
            opt.state[q] = dict(step=torch.tensor(float(first_gstep)), exp_avg=torch.zeros_like(q),
                                exp_avg_sq=torch.zeros_like(q))
        losses = []
        for s in range(math.ceil(n_items / B)):
            rows = idx[s * B:(s + 1) * B]
            opt.zero_grad()
            l = ref.loss(X[rows], Y[rows], first_gstep + s, loss)
            l.backward()
            opt.step()
            losses.append(float(l.detach()))
        params = list(ref.net.parameters())
        return (torch.tensor(losses, dtype=torch.float64),
                torch.cat([opt.state[q]["exp_avg"].reshape(-1) for q in params]),
                torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in params]))
    return run


def _check_trajectory(p, m, v, losses, ref, ref_losses, ref_m, ref_v):
    """The project's trajectory bounds, asserted by test_mlp_tile_gpu._check_against_torch itself (parameters,
    losses, m and v).  It compares fp32 tensors, so the fp64 reference is rounded to fp32 for it: 6e-8
    relative, against bounds of 1e-3 relative and more.  The worst raw errors are printed from the fp64 values."""
    print("worst errors vs fp64: loss %.3e, m %.3e, v %.3e"
          % ((losses.double().cpu() - ref_losses).abs().max(), (m.double().cpu() - ref_m).abs().max(),
             (v.double().cpu() - ref_v).abs().max()))
    assert torch.isfinite(p).all()
    _check_against_torch(p, m, v, losses, ref.net, ref_losses.float(), ref_m.float(), ref_v.float())


TRAJECTORIES = [([5, 64, 2], 4, NO_ENV, "wave_rows"), ([9, 48, 64, 3], 4, NO_ENV, "wave_single"),
                ([5, 128, 128, 2], 4, NO_ENV, "block5"), ([5, 128, 128, 2], 8, NO_ENV, "block5_b8"),
                ([5, 128, 128, 2], 4, BLOCK3, "block3")]


@pytest.mark.parametrize("loss", ["ce", "mse"])
@pytest.mark.parametrize("dims,B,env,trainer", TRAJECTORIES, ids=_ids(TRAJECTORIES, family=True))
def test_trajectory_matches_fp64_adam_under_host_mask(dims, B, env, trainer, loss, cuda, monkeypatch):
    """7 steps in two launches (3, then 4 at t0 = step_base = 3), the last batch partial: [5,64,2] runs
    wave_rows_x0, [9,48,64,3] the single-wave kernel, 3x128 mlp_block5 (B = 8: mlp_block5_b8) or mlp_block3."""
    n_items = (STEPS - 1) * B + B - 1
    k = _kernel(dims, B, env, monkeypatch)
    _check_plan(k, B, trainer, mode=0)
    X, Y, idx, net, ref, want = _build(dims, B, n_items, k, _adam_reference(B, n_items, 0, loss))
    p = _flat(net).to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(STEPS, device=cuda)
    Xd, Yd, idxd = X.to(cuda), Y.to(cuda, torch.int32), idx.to(cuda, torch.int32)
    for first, n in ((0, 3), (3, 4)):
        k.train(p, m, v, Xd, Yd, idxd[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=first,
                step_base=first, lr=LR, dropout=PDROP, seed=SEED, loss=loss, loss_out=losses[first:])
    torch.cuda.synchronize()
    _check_trajectory(p, m, v, losses, ref, *want)


def test_bound_train_mask_step_follows_the_device_counter(cuda, monkeypatch):
    """prepare_train / BoundTrain.run with a device step counter that starts at 9: Adam's step and the
    mask's step are the counter's (9 .. 15), not the launch's first step."""
    dims, B, first_gstep = [5, 64, 2], 4, 9
    n_items = (STEPS - 1) * B + B - 1
    k = _kernel(dims, B, NO_ENV, monkeypatch)
    _check_plan(k, B, "wave_rows", mode=0)
    X, Y, idx, net, ref, want = _build(dims, B, n_items, k, _adam_reference(B, n_items, first_gstep, "ce"))
    p = _flat(net).to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(STEPS, device=cuda)
    counter = torch.full((1,), first_gstep, dtype=torch.int32, device=cuda)
    bound = k.prepare_train(p, m, v, X.to(cuda), Y.to(cuda, torch.int32), idx.to(cuda, torch.int32), n_items=n_items,
                            batch=B, lr=LR, dropout=PDROP, seed=SEED, loss_out=losses, step_counter=counter)
    bound.run(0, 3)
    bound.run(3, 4)
    torch.cuda.synchronize()
    assert int(counter.item()) == first_gstep + STEPS
    _check_trajectory(p, m, v, losses, ref, *want)
