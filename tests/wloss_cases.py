"""Class-weighted, label-smoothed cross-entropy in the batch-tiled MLP path (csrc/mlp_tile.hip, csrc/mlp_infer.hip):
the cases the GPU tests run, their fp64 reference, the wrong implementations the tolerances must reject, and the
inference bound.

For live rows i, class weights w[c] > 0 and smoothing eps in [0, 1) - torch's
``F.cross_entropy(weight=, label_smoothing=)``:

    t[i][c] = (1 - eps) w[y_i] [c == y_i] + (eps / C) w[c]
    num_i   = -sum_c t[i][c] log_softmax(z_i)[c]
    W       = sum_i w[y_i]
    loss    = sum_i num_i / W
    dloss/dz[i][k] = (softmax(z_i)[k] sum_c t[i][c] - t[i][k]) / W

``CASES``: (dims, batch) - the smallest shapes at which the tile logic can go wrong (two tiles with one live row in
the second, three tiles with C = 3, C = 4, and batch 4 on the tile plan), each over ``n_items = 2 B + 5`` index
entries, so the last step has 5 rows (1 row at batch 4) and whole tiles without a live row.  ``VARIANTS``: weights
only, smoothing only, both.
Weights spread over [0.5, 4]; labels imbalanced (class c about twice as frequent as class c + 1, so W is far from the
row count) and arranged so that every class appears in every tile that has at least C live rows.

``reference(case, variant, step, mutant=None)``: everything in fp64 from the case's fp32 inputs.  The gradient goes
through a plain fp64 MLP with the dlogits of the formula above as the backward seed - torch's own cross-entropy is
not part of it (tests/test_wloss_cases_cpu.py compares the two).  ``MUTANTS`` are the four wrong implementations.

``infer_reference(case, variant)``: sum_i num_i over all n_items rows and its bound, built from
tests/infer_cases.py's logit bound and CE row bound: num_i = sum_c t[c] (lse - z_c), every term is a CE row loss for
label c (bound_loss_c) scaled by t[c]; t[c] costs at most 3 roundings (the two products and the fused add), the
product and the <= 4-term fused sum at most 5 more: 16 u |num_i| covers them.  Nothing comes from a kernel's output.

A plain module, not a conftest: the tests import it."""
import functools

import torch

import infer_cases as ic

R = 32  # rows per tile
CASES = [([5, 64, 2], 17), ([5, 64, 2], 40), ([7, 48, 32, 3], 65), ([32, 128, 128, 4], 17), ([5, 64, 2], 4)]
VARIANTS = {"w": (True, 0.0), "s": (False, 0.1), "ws": (True, 0.1)}  # name -> (class weights on, eps)
MUTANTS = ["norm_bs", "unweighted_smooth", "w_counts_pad", "dropped_1m_eps"]
# the variants in which a mutant computes something else than the feature (smoothing alone has w = 1, so W = bs and
# the smoothing term has nothing to weight; without smoothing there is no (1 - eps))
MUTANT_VARIANTS = {"norm_bs": ("w", "ws"), "unweighted_smooth": ("ws",), "w_counts_pad": ("w", "s", "ws"),
                   "dropped_1m_eps": ("s", "ws")}
GRAD_ATOL, GRAD_RTOL, LOSS_ATOL = 1e-6, 1e-4, 1e-5  # test_mlp_tile_gpu.py::test_tile_grad_mode_matches_autograd's


def case_id(case):
    dims, B = case
    return ic.name(dims) + f"-b{B}"


def n_items_of(B, k=2):
    """k full batches and 5 rows (the one-step and inference checks: k = 2; the 7-step training runs: k = 6)."""
    return k * B + 5


def n_steps(B, k=2):
    return -(-n_items_of(B, k) // B)


def grad_steps(case):
    """The steps the one-step checks run: the full first batch, and the last one (5 rows; 1 row at batch 4), whose
    other tiles are empty."""
    return (0, n_steps(case[1]) - 1)


def class_weights(C):
    """fp32 [C] over [0.5, 4]."""
    return torch.linspace(0.5, 4.0, C, dtype=torch.float32)


def variant_args(variant, C):
    """(class weights fp32 [C] or None, eps) of a variant."""
    on, eps = VARIANTS[variant]
    return (class_weights(C) if on else None), eps


@functools.lru_cache(maxsize=None)
def _inputs(dims, B, k):
    C = dims[-1]
    n_items = n_items_of(B, k)
    g = torch.Generator().manual_seed(4000 + 17 * B + dims[0] + 1000 * k)
    parts = []
    for l in range(len(dims) - 1):
        i, o = dims[l], dims[l + 1]
        s = 2.0 / i ** 0.5
        parts += [(torch.rand(o, i, generator=g) * 2 - 1) * s, (torch.rand(o, generator=g) * 2 - 1) * s]
    p = torch.cat([t.reshape(-1) for t in parts]).float()
    N = n_items + 37
    X = torch.randn(N, dims[0], generator=g).float()
    idx = torch.randperm(N, generator=g)[:n_items].to(torch.int32)
    # labels in visiting order: imbalanced draws, then every tile of every batch with >= C live rows opens with one
    # row of each class
    probs = torch.tensor([2.0 ** -c for c in range(C)])
    seq = torch.multinomial(probs, n_items, replacement=True, generator=g)
    for first in range(0, n_items, B):
        bs = min(B, n_items - first)
        for r0 in range(0, bs, R):
            if min(R, bs - r0) >= C:
                seq[first + r0: first + r0 + C] = torch.randperm(C, generator=g)
    Y = torch.randint(0, C, (N,), generator=g, dtype=torch.int32)
    Y[idx.long()] = seq.to(torch.int32)
    return dict(p=p, X=X, Y=Y, idx=idx)


def inputs(case, k=2):
    """The case's fp32 / integer inputs on the CPU: p (flat, torch state_dict order), X [N, D0], Y int32 [N],
    idx int32 [n_items_of(B, k)] (a permutation prefix: no row twice)."""
    dims, B = case
    return _inputs(tuple(dims), B, k)


def step_rows(case, step):
    """(x fp32 [bs, D0], y int64 [bs]) of optimizer step ``step``, in batch order."""
    dims, B = case
    d = inputs(case)
    sel = d["idx"][step * B: (step + 1) * B].long()
    return d["X"][sel], d["Y"][sel].long()


def target_mass(y, w, eps, C, mutant=None):
    """t [n, C] in the dtype of ``w``."""
    onehot = torch.nn.functional.one_hot(y, C).to(w.dtype)
    on = onehot * w[y][:, None]
    if mutant != "dropped_1m_eps":
        on = (1.0 - eps) * on
    smooth = (eps / C) * (torch.ones_like(w) if mutant == "unweighted_smooth" else w)
    return on + smooth[None, :]


def row_terms(z, y, w, eps, mutant=None):
    """(num [n], t [n, C], dlogits before the normaliser [n, C]) from logits z, all in z's dtype."""
    C = z.shape[1]
    t = target_mass(y, w.to(z.dtype), eps, C, mutant)
    logp = torch.log_softmax(z, 1)
    num = -(t * logp).sum(1)
    dz = torch.softmax(z, 1) * t.sum(1, keepdim=True) - t
    return num, t, dz


def normaliser(y, w, B_pad=0, mutant=None):
    """W = sum_i w[y_i] (fp64).  Mutants: the row count; or counting the dead rows of the last tile, whose label
    slot the kernel fills with 0."""
    if mutant == "norm_bs":
        return float(len(y))
    W = float(w.double()[y].sum())
    if mutant == "w_counts_pad":
        W += B_pad * float(w[0])
    return W


def forward64(dims, p, x):
    """fp64 logits of the flat-parameter MLP (ReLU between layers), differentiable in ``p``."""
    a = x.double()
    layers = ic.split_params(p, dims)
    for l, (Wl, b) in enumerate(layers):
        a = a @ Wl.t() + b
        if l < len(layers) - 1:
            a = torch.relu(a)
    return a


@functools.lru_cache(maxsize=None)
def _reference(dims, B, variant, step, mutant):
    case = (list(dims), B)
    C = dims[-1]
    w, eps = variant_args(variant, C)
    w = torch.ones(C) if w is None else w
    x, y = step_rows(case, step)
    p = inputs(case)["p"].double().requires_grad_()
    z = forward64(list(dims), p, x)
    num, t, dz = row_terms(z.detach(), y, w.double(), eps, mutant)
    pad = (-len(y)) % R
    W = normaliser(y, w, pad, mutant)
    z.backward(dz / W)
    return dict(loss=float(num.sum() / W), grads=p.grad.detach().clone(), W=W, num=num, dlogits=dz / W,
                logits=z.detach(), y=y)


def reference(case, variant, step, mutant=None):
    """fp64: dict(loss, grads [P], W, num [bs], dlogits [bs, C], logits [bs, C], y)."""
    dims, B = case
    return _reference(tuple(dims), B, variant, step, mutant)


def grads_inside(got, ref):
    """The grad-mode check of the GPU test: (gradients inside, loss inside)."""
    g_ok = torch.allclose(got["grads"].double(), ref["grads"], atol=GRAD_ATOL, rtol=GRAD_RTOL)
    return bool(g_ok), abs(float(got["loss"]) - ref["loss"]) < LOSS_ATOL


@functools.lru_cache(maxsize=None)
def _infer_reference(dims, B, variant):
    case = (list(dims), B)
    C = dims[-1]
    d = inputs(case)
    w, eps = variant_args(variant, C)
    w = torch.ones(C) if w is None else w
    sel = d["idx"].long()
    x, y = d["X"][sel], d["Y"][sel].long()
    z, bz = ic.forward64(list(dims), d["p"], x)
    num, t, _ = row_terms(z, y, w.double(), eps)
    # CE row bound for every possible label c, scaled by the target mass on c
    bound = torch.zeros_like(num)
    for c in range(C):
        bound += t[:, c] * ic.stats64(z, bz, torch.full_like(y, c), "ce")["bound_loss"]
    bound += 16 * ic.U * num.abs()
    pred = z.argmax(1)
    top2 = z.topk(2, dim=1).values
    ambiguous = (top2[:, 0] - top2[:, 1]) < 2 * bz.max(1).values
    return dict(num_sum=float(num.sum()), bound=float(bound.sum()), W=float(w.double()[y].sum()), y=y, pred=pred,
                ambiguous=ambiguous, n=len(y))


def infer_reference(case, variant):
    """fp64 over all n_items rows: dict(num_sum, bound, W, y, pred, ambiguous, n)."""
    dims, B = case
    return _infer_reference(tuple(dims), B, variant)
