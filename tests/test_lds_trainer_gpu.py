"""Every instantiation of the generic LDS trainer (csrc/mlp_fused_impl.h ``mlp_train_kernel<L, NT, MAXQ, BMAX,
BR>``, 42 kernels) and of ``mlp_eval_kernel`` against float64 references (run on a real MI355X).

The shapes are tests/lds_cases.py's table, which tests/test_lds_cases_cpu.py proves complete; the float64
reference under the host mirror's dropout masks, the ReLU-margin seed search and the tolerances are
tests/test_dropout_reference_gpu.py's.  Every case asserts the plan's ownership class and the trainer "lds"
before it launches, and every instantiation has its own test id: a failure names one kernel."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import dct_amd  # noqa: F401
from dct_amd.ops.fused_mlp import FusedMLPKernel

import lds_cases
from test_dropout_reference_gpu import (LR, PDROP, SEED, STEPS, P32, _adam_reference, _build, _check_plan,
                                        _check_trajectory, _excess, _flat, _fresh_knobs, _grad_case, _kernel,  # noqa: F401
                                        _ref_net, _Reference, _train_step_case, _with_siblings)

pytestmark = pytest.mark.gpu

ENV = lds_cases.ENV
LOSSES = ("ce", "mse")
M_ATOL, M_RTOL = 1e-4, 1e-2  # test_mlp_tile_gpu._check_against_torch's bound on m (and on v)
WEIGHT_DECAY = 0.05


def _cls_name(cls):
    return "%dx%dx%d" % cls


def _assert_class(dims, B, cls, monkeypatch):
    """The launch of this case reaches the instantiation it is named after."""
    k = _kernel(dims, B, ENV, monkeypatch)
    assert (k.plan.threads, k.plan.max_blocks_per_thread, k.plan.block_rows) == cls
    assert k.plan.bmax == (4 if B <= 4 else 16)
    assert k.plan.trainer(B, mode=0) == k.plan.trainer(B, mode=1) == "lds"
    return k


# ------------------------------------------------------------------ a. grad mode and one Adam step
def _step_cases():
    """(dims, class, B, n_items, loss): every table row at both batch limits, full and partial batches; the
    loss alternates over the table (each class has a row of either loss at each batch limit), edge rows
    get both."""
    out = []
    for i, (dims, cls) in enumerate(lds_cases.TABLE):
        for bi, batches in enumerate(((4, 1), (16, 9))):
            for d, B, n, _ in _with_siblings([(dims, B, ENV) for B in batches]):
                out.append((d, cls, B, n, LOSSES[(i + bi) % 2]))
    for dims, bmaxes, cls, batch, _ in lds_cases.EDGES:
        for bmax in bmaxes:
            batches = (batch,) if batch else ((4, 1) if bmax == 4 else (16, 9))
            for d, B, n, _ in _with_siblings([(dims, B, ENV) for B in batches]):
                out += [(d, cls, B, n, loss) for loss in LOSSES]
    return out


def _step_id(c):
    dims, cls, B, n, loss = c
    return "L%d-%s-bmax%d-B%dof%d-%s-%s" % (len(dims) - 1, _cls_name(cls), 4 if B <= 4 else 16, n, B, loss,
                                            lds_cases.name(dims))


STEP_CASES = _step_cases()


@pytest.mark.parametrize("dims,cls,B,n_items,loss", STEP_CASES, ids=[_step_id(c) for c in STEP_CASES])
def test_lds_grad_mode_matches_fp64(dims, cls, B, n_items, loss, cuda, monkeypatch):
    _assert_class(dims, B, cls, monkeypatch)
    _grad_case(dims, B, n_items, ENV, loss, "lds", cuda, monkeypatch)


@pytest.mark.parametrize("dims,cls,B,n_items,loss", STEP_CASES, ids=[_step_id(c) for c in STEP_CASES])
def test_lds_train_step_matches_fp64(dims, cls, B, n_items, loss, cuda, monkeypatch):
    _assert_class(dims, B, cls, monkeypatch)
    _train_step_case(dims, B, n_items, ENV, loss, "lds", cuda, monkeypatch)


# ------------------------------------------------------------------ b. trajectories
class _Reference32(_Reference):
    """The same net under the same masks in plain fp32 torch: what fp32 arithmetic alone costs."""

    def __init__(self, net32, k, B):
        super().__init__(net32, k, B)
        self.net = copy.deepcopy(net32)
        self.lins = [l for l in self.net if isinstance(l, torch.nn.Linear)]

    def loss(self, x, y, gstep, kind):
        h = x.float()
        for li, lin in enumerate(self.lins[:-1]):
            keep = self.k.dropout_mask(SEED, gstep, li, self.B, PDROP)[:x.shape[0]]
            h = torch.relu(lin(h)) * keep * torch.tensor(1.0 / (1.0 - P32), dtype=torch.float32)
        logits = self.lins[-1](h)
        if kind == "ce":
            return F.cross_entropy(logits, y)
        return F.mse_loss(logits, F.one_hot(y, logits.shape[1]).float())


def _adam(B, n_items, first_gstep, loss, weight_decay):
    """_adam_reference, with torch.optim.Adam's (coupled) weight decay where the case has one."""
    if not weight_decay:
        return _adam_reference(B, n_items, first_gstep, loss)

    def run(ref, X, Y, idx):
        opt = torch.optim.Adam(ref.net.parameters(), lr=LR, weight_decay=weight_decay)
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


def _sqrt_v_ratio(got_v, ref_v):
    """Worst |sqrt(v) - sqrt(v64)| over m's bound 1e-4 + 1e-2 sqrt(v64): sqrt(v) has m's scale."""
    want = ref_v.double().sqrt()
    return float(((got_v.double().cpu().sqrt() - want).abs() / (M_ATOL + M_RTOL * want)).max())


def _trajectory_problem(dims, B, loss, first_gstep, weight_decay, monkeypatch):
    n_items = (STEPS - 1) * B + B - 1
    k = _kernel(dims, B, ENV, monkeypatch)
    _check_plan(k, B, "lds", mode=0)
    return (k, n_items) + _build(dims, B, n_items, k, _adam(B, n_items, first_gstep, loss, weight_decay))


def fp32_reference_sqrt_v_ratio(dims, B, loss, weight_decay, monkeypatch, first_gstep=0):
    """The ratio of _sqrt_v_ratio for the fp32 torch reference of a trajectory case (no GPU): the measurement
    behind SQRT_V_BOUND, asserted by tests/test_lds_cases_cpu.py."""
    k, n_items, X, Y, idx, net, _, (_, _, ref_v) = _trajectory_problem(dims, B, loss, first_gstep, weight_decay,
                                                                       monkeypatch)
    _, _, v32 = _adam(B, n_items, first_gstep, loss, weight_decay)(_Reference32(net, k, B), X, Y, idx)
    return _sqrt_v_ratio(v32, ref_v)


# The plain fp32 torch reference of every trajectory case below (TRAJECTORIES x both losses, DECAYED, the
# bound launch) stays under FP32_RATIO_LIMIT of m's bound: 6.2e-4 of it at worst (see
# test_lds_trajectory_matches_fp64_adam's docstring), so sqrt(v) is held to m's bound itself.
FP32_RATIO_LIMIT = 0.25
SQRT_V_BOUND = 1.0


def _check_sqrt_v(v, ref_v):
    r = _sqrt_v_ratio(v, ref_v)
    print("worst |sqrt(v) - sqrt(v64)| / (1e-4 + 1e-2 sqrt(v64)): %.4f of %.2f" % (r, SQRT_V_BOUND))
    assert r <= SQRT_V_BOUND, r


def _run_trajectory(dims, B, loss, weight_decay, cuda, monkeypatch):
    k, n_items, X, Y, idx, net, ref, want = _trajectory_problem(dims, B, loss, 0, weight_decay, monkeypatch)
    p = _flat(net).to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(STEPS, device=cuda)
    Xd, Yd, idxd = X.to(cuda), Y.to(cuda, torch.int32), idx.to(cuda, torch.int32)
    for first, n in ((0, 3), (3, 4)):
        k.train(p, m, v, Xd, Yd, idxd[first * B:], n_items=n_items - first * B, batch=B, steps=n, t0=first,
                step_base=first, lr=LR, weight_decay=weight_decay, dropout=PDROP, seed=SEED, loss=loss,
                loss_out=losses[first:])
    torch.cuda.synchronize()
    assert torch.isfinite(m).all() and torch.isfinite(v).all() and bool((v >= 0).all())
    _check_trajectory(p, m, v, losses, ref, *want)
    _check_sqrt_v(v, want[2])


# the smallest row of each ownership class at both batch limits, and the batch-prefetch edges (whose two
# paths differ only from the second step of a launch on)
TRAJECTORIES = ([(d, cls, B) for d, cls in zip(lds_cases.smallest_per_class(), lds_cases.CLASSES) for B in (4, 16)]
                + [(e[0], e[2], e[3]) for e in lds_cases.EDGES if e[3]])
DECAYED = [([1, 26, 30, 3], (256, 2, 1), 4), ([11, 74, 38, 3], (256, 2, 4), 16)]  # a br = 1 and a br = 4 row
COUNTER_CASE = (lds_cases.smallest_per_class()[5], (512, 3, 4), 16)  # a 512-thread row


def _traj_id(c):
    dims, cls, B = c
    return "L%d-%s-bmax%d-%s" % (len(dims) - 1, _cls_name(cls), 4 if B <= 4 else 16, lds_cases.name(dims))


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("dims,cls,B", TRAJECTORIES, ids=[_traj_id(c) for c in TRAJECTORIES])
def test_lds_trajectory_matches_fp64_adam(dims, cls, B, loss, cuda, monkeypatch):
    """7 steps in two launches (3, then 4 at t0 = step_base = 3), the last batch partial: the second launch
    reloads its register-resident moments from m / v.

    On top of _check_trajectory's bounds, sqrt(v) is compared with sqrt(v64): v's own bound (atol 1e-4) is
    larger than v, so it cannot see a bad reload of v; sqrt(v) has m's scale.  Its bound comes from the plain
    fp32 torch reference of the same trajectories on the CPU (fp32_reference_sqrt_v_ratio), never from the
    kernel: over these cases, the weight-decay ones and the bound launch, the fp32 reference's worst
    |sqrt(v) - sqrt(v64)| / (1e-4 + 1e-2 sqrt(v64)) measured 6.2e-4 at worst ([31,138,150,2] CE; 4.6e-4 on
    [17,138,150,2] MSE at batch 4, 1.8e-4 on the bound launch, 1e-5 on every row narrower than 98 units and on
    the weight-decay cases).  That is far under a quarter of m's bound, so m's bound (atol 1e-4, rtol 1e-2)
    is the one asserted; tests/test_lds_cases_cpu.py re-measures the quarter without a GPU."""
    _assert_class(dims, B, cls, monkeypatch)
    _run_trajectory(dims, B, loss, 0.0, cuda, monkeypatch)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("dims,cls,B", DECAYED, ids=[_traj_id(c) for c in DECAYED])
def test_lds_trajectory_with_weight_decay_matches_fp64_adam(dims, cls, B, loss, cuda, monkeypatch):
    """The same trajectory with weight_decay = 0.05 against fp64 torch.optim.Adam(weight_decay=0.05): the
    trainer's ``g += wd * p`` on weights and biases."""
    _assert_class(dims, B, cls, monkeypatch)
    _run_trajectory(dims, B, loss, WEIGHT_DECAY, cuda, monkeypatch)


def test_lds_bound_train_follows_the_device_counter(cuda, monkeypatch):
    """prepare_train / BoundTrain.run with a device step counter that starts at 9, on a 512-thread plan:
    Adam's step and the mask's step are the counter's (9 .. 15), not the launch's first step."""
    dims, cls, B = COUNTER_CASE
    first_gstep = 9
    _assert_class(dims, B, cls, monkeypatch)
    k, n_items, X, Y, idx, net, ref, want = _trajectory_problem(dims, B, "ce", first_gstep, 0.0, monkeypatch)
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
    _check_sqrt_v(v, want[2])


# ------------------------------------------------------------------ c. evaluation kernel
EVAL_ROWS = [[30, 222, 5], [17, 138, 150, 2], [1, 42, 90, 38, 6]]  # [17,138,150,2]: a 512-thread plan run by 256
EVAL_N = (1, 15, 16, 17, 777)
EVAL_GRIDS = (1, None, 64)  # None: the launcher's default; 64 exceeds the chunk count at 17 rows
EVAL_SEEDS = range(60, 92)
EVAL_GAP = 1e-4
EVAL_LOSS_TOL = 1.3e-5  # per row: test_fused_eval_matches_torch's 1e-2 at 777 rows


@functools.lru_cache(maxsize=None)
def eval_problem(dims, n_max=777):
    """(X, Y, idx, fp32 net, fp64 logits of the n_max indexed rows) of the first seed whose fp64 top-two
    logit gap exceeds EVAL_GAP on every row: the kernel's fp32 rounding cannot change an argmax.  Computed
    once per shape and shared (never modified) by the cases; smaller cases take a prefix of idx."""
    dims = list(dims)
    for s in EVAL_SEEDS:
        torch.manual_seed(s)
        N = n_max + 223
        X = torch.randn(N, dims[0])
        Y = torch.randint(0, dims[-1], (N,))
        idx = torch.randperm(N)[:n_max]
        net = _ref_net(dims)
        with torch.no_grad():
            z = copy.deepcopy(net).double()(X[idx].double())
        top = z.topk(2, dim=1).values
        gap = float((top[:, 0] - top[:, 1]).min())
        if gap > EVAL_GAP:
            print("eval seed %d, smallest top-two gap %.3e" % (s, gap))
            return X, Y, idx, net, z
    pytest.fail("no seed in %r keeps every row's top-two logits %g apart" % (EVAL_SEEDS, EVAL_GAP))


def _eval_reference(z, y, loss):
    if loss == "ce":
        total = F.cross_entropy(z, y, reduction="sum")
    else:
        total = F.mse_loss(z, F.one_hot(y, z.shape[1]).double(), reduction="sum") / z.shape[1]
    return float(total), int((z.argmax(1) == y).sum())


def _check_eval(k, p, problem, z, n_items, grid, loss, cuda):
    X, Y, idx = problem
    C = z.shape[1]
    acc = torch.zeros(2, device=cuda)
    logits = torch.full((n_items * C,), float("nan"), device=cuda)
    args = (p, X.to(cuda), Y.to(cuda, torch.int32), idx[:n_items].to(cuda, torch.int32), n_items, acc)
    k.evaluate(*args, loss=loss, logits_out=logits, grid=grid)
    torch.cuda.synchronize()
    once = acc.cpu().clone()
    want_loss, want_corr = _eval_reference(z[:n_items], Y[idx[:n_items]], loss)
    assert _excess(logits.view(n_items, C), z[:n_items], 1e-4, 1e-4) <= 0
    print("summed loss %.6f, fp64 %.6f (tolerance %.2e); correct %d of %d"
          % (float(once[0]), want_loss, EVAL_LOSS_TOL * n_items, int(once[1]), n_items))
    assert abs(float(once[0]) - want_loss) <= EVAL_LOSS_TOL * n_items
    assert float(once[1]) == want_corr
    # no reset: a second call adds the same sums
    k.evaluate(*args, loss=loss, grid=grid)
    torch.cuda.synchronize()
    twice = acc.cpu()
    assert float(twice[1]) == 2 * want_corr
    assert abs(float(twice[0]) - 2 * want_loss) <= 2 * EVAL_LOSS_TOL * n_items
    if grid == 1:  # one workgroup, one atomic per entry: exactly twice
        assert float(twice[0]) == 2 * float(once[0])


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("grid", EVAL_GRIDS, ids=["grid1", "griddefault", "grid64"])
@pytest.mark.parametrize("n_items", EVAL_N)
@pytest.mark.parametrize("dims", EVAL_ROWS, ids=["L%d-%s" % (len(d) - 1, lds_cases.name(d)) for d in EVAL_ROWS])
def test_lds_eval_matches_fp64(dims, n_items, grid, loss, cuda, monkeypatch):
    """mlp_eval_kernel<L, 256, 16> per depth: logits, summed loss, exact correct count, accumulation."""
    k = _kernel(dims, 16, ENV, monkeypatch)
    assert k.eval_plan.bmax == 16
    X, Y, idx, net, z = eval_problem(tuple(dims))
    _check_eval(k, _flat(net).to(cuda), (X, Y, idx), z, n_items, grid, loss, cuda)


# ------------------------------------------------------------------ d. whatever trains can validate
VALIDATE_EDGE = [[21, 164, 164, 5], [14, 116, 116, 116, 5]]  # their 16-row layout overflows the LDS budget


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("dims", VALIDATE_EDGE, ids=[lds_cases.name(d) for d in VALIDATE_EDGE])
def test_supported_shape_can_validate(dims, loss, cuda, monkeypatch):
    """Shapes ``FusedMLPKernel.supported`` accepts at batch 4 only: one training step, then ``evaluate`` (which
    used to build a 16-row plan the evaluation launcher refused), both against fp64.  The evaluation runs
    mlp_eval_kernel<L, 256, 4> on the trained parameters; its reference is their fp64 forward."""
    B = 4
    assert FusedMLPKernel.supported(dims, B) and not FusedMLPKernel.supported(dims, 16)
    _train_step_case(dims, B, B, ENV, loss, "lds", cuda, monkeypatch)
    k = _kernel(dims, B, ENV, monkeypatch)
    assert k.eval_plan.bmax == 4
    X, Y, idx, net, _ = eval_problem(tuple(dims), 45)
    p = _flat(net).to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    k.train(p, m, v, X.to(cuda), Y.to(cuda, torch.int32), idx.to(cuda, torch.int32), n_items=B, batch=B, steps=1,
            t0=0, lr=LR, dropout=PDROP, seed=SEED, loss=loss)
    torch.cuda.synchronize()
    assert float((p.cpu() - _flat(net)).abs().max()) > 1e-3  # the step moved the parameters
    trained = _ref_net(dims).double()
    torch.nn.utils.vector_to_parameters(p.cpu().double(), trained.parameters())
    with torch.no_grad():
        z = trained(X[idx].double())
    # the trained parameters exist only now: keep the rows whose fp64 top-two gap on them exceeds EVAL_GAP
    top = z.topk(2, dim=1).values
    keep = torch.nonzero(top[:, 0] - top[:, 1] > EVAL_GAP).flatten()
    keep = keep[:len(keep) - 1] if len(keep) % 4 == 0 else keep  # the last 4-row chunk stays partial
    assert len(keep) >= 40
    for n_items, grid in ((len(keep), None), (len(keep), 1), (3, 64)):  # >= 10 chunks of 4; one chunk, 64 groups
        _check_eval(k, p, (X, Y, idx[keep]), z[keep], n_items, grid, loss, cuda)


def test_engine_validates_the_model_it_accepts(cuda):
    """The path that failed: ``FusedMLPEngine.applicable`` takes [21,164,164,5] at batch 4, trains it, and its
    first ``validate()`` raised ``mlp_eval failed`` (a 16-row evaluation plan of 178,880 B)."""
    from dct_amd.models.mlp import MLPClassifier
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import FusedMLPEngine, adam_hparams_from

    torch.manual_seed(0)
    model = MLPClassifier(21, hidden=(164, 164), num_classes=5, dropout=0.0)
    assert FusedMLPEngine.applicable(model, cuda, 4) and not FusedMLPEngine.applicable(model, cuda, 16)
    X, Y, rows = torch.randn(200, 21), torch.randint(0, 5, (200,)), torch.randperm(200)
    eng = FusedMLPEngine(model, init_distributed("gpu"), 4, seed=42,
                         adam=adam_hparams_from(model.configure_optimizers()))
    assert eng.kernel.plan.trainer(4) == "lds"
    eng.attach_data(X, Y, rows[:160], rows[160:])
    n = eng.upload_epoch_indices(0)
    losses = torch.zeros(8, device=cuda)
    eng.run_steps(n, 5, losses)
    val_loss, val_acc = eng.validate()
    trained = _ref_net([21, 164, 164, 5]).double()
    torch.nn.utils.vector_to_parameters(eng.p.cpu().double(), trained.parameters())
    with torch.no_grad():
        z = trained(X[rows[160:]].double())
    want_loss, want_corr = _eval_reference(z, Y[rows[160:]], "ce")
    top = z.topk(2, dim=1).values
    close = int((top[:, 0] - top[:, 1] <= EVAL_GAP).sum())  # rows whose argmax fp32 rounding may change
    assert torch.isfinite(losses[:5]).all()
    assert abs(val_loss - want_loss / 40) <= EVAL_LOSS_TOL
    assert abs(val_acc * 40 - want_corr) <= close + 1e-3
