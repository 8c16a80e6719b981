"""The batch-tiled inference kernel's (csrc/mlp_infer.hip) test cases, their fp64 reference and the error bounds.

``CASES``: every shape x every row count below, index lists alternating between ``None`` and a permutation with
duplicates, losses between CE and MSE, plus the special cases (logits of +-100, normalisation with a zero-std column).

``reference(case)`` computes everything in fp64 from the case's fp32 inputs and derives the bounds from fp64
quantities only - nothing is hand-picked, nothing comes from what the kernel returns:

  * logits: layer l adds ``(K_l + 2) u sum_k |w_ok| (|a_k| + e_k) + |b_o|`` of rounding (u = 2^-24; the kernel's chains
    have at most K_l + 1 roundings: K_l fused multiply-adds and the bias, or K_l / 8 + 4 in the head's 8-way split) and
    carries the incoming error ``sum_k |w_ok| e_k`` through; ReLU is 1-Lipschitz.  With ``norm`` the input starts
    at ``e = (2 u + 4 u^2) |x_n|`` (one rounding in x - mean, one in the correctly rounded division).
  * probabilities: with d = max_c bound_z + u (max_c (mx - z_c) + 2 max_c bound_z) (the logit error and the rounding
    of z_c - mx), exact softmax moves by at most p (e^{2d} - 1); exp (<= 2 ulp), the sum of <= 4 terms and the division
    add at most 16 u relative; 2^-126 covers results in the subnormal range.
  * row loss: CE = mx + log(sum) - z_y: 2 max_c bound_z + 16 u + 4 u (|mx| + |z_y| + 2);
    MSE = mean_c d_c^2: mean_c (2 |d_c| bound_c + bound_c^2) + 8 u mean_c d_c^2 + 2^-126.  The loss sum's bound is the
    sum of its rows' (the kernel adds the rows in fp64).
  * argmax / confusion comparisons leave out rows whose fp64 top-2 gap is below twice the row's logit bound - at most
    2 % of a case's rows (``MAX_AMBIGUOUS``); tests/test_infer_cases_cpu.py checks every case's seed against the cap.

``emulate(case, mutant=None)`` is a torch fp32 emulation of the kernel's accumulation order (fused multiply-adds as
fp64 product + sum rounded to fp32), with the mutants the CPU test must see fail.

A plain module, not a conftest: the tests import it."""
import functools

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
MAX_AMBIGUOUS = 0.02
R = 32  # rows per tile

SHAPES = [[5, 64, 2], [5, 128, 128, 2], [7, 48, 32, 3], [32, 128, 128, 4], [1, 16, 16, 2]]
# (rows, grid): 165 rows are six tiles - three per workgroup with the last one partial at grid 2, mostly idle
# workgroups at grid 64
ROWS = [(1, None), (31, None), (32, None), (33, None), (165, 2), (165, 64)]


# seeds replaced because the fp64 reference alone had more near-tied rows than the cap allows (31 rows allow none)
_SEEDS = {(3, 1): 3031}


def name(dims):
    return "x".join(str(d) for d in dims)


def _table():
    out = []
    for i, dims in enumerate(SHAPES):
        for k, (n, grid) in enumerate(ROWS):
            out.append(dict(name=f"{name(dims)}-n{n}" + (f"-g{grid}" if grid else ""), dims=dims, n=n, grid=grid,
                            idx="dup" if (i + k) % 2 else None, loss="mse" if (i + k) % 3 == 0 else "ce",
                            norm=False, head_scale=1.0, seed=_SEEDS.get((i, k), 1000 + 10 * i + k)))
    # logits reach +-100: a softmax without the maximum subtracted overflows
    out.append(dict(name="5x64x2-n165-logits100", dims=[5, 64, 2], n=165, grid=None, idx=None, loss="ce", norm=False,
                    head_scale=400.0, seed=2001))
    out.append(dict(name="5x128x128x2-n165-logits100", dims=[5, 128, 128, 2], n=165, grid=None, idx="dup", loss="ce",
                    norm=False, head_scale=400.0, seed=2002))
    # raw inputs normalised in the gather; column 1's std is 0 (replaced by 1 before upload)
    out.append(dict(name="5x64x2-n165-norm", dims=[5, 64, 2], n=165, grid=None, idx="dup", loss="ce", norm=True,
                    head_scale=1.0, seed=2003))
    out.append(dict(name="7x48x32x3-n33-norm", dims=[7, 48, 32, 3], n=33, grid=None, idx=None, loss="mse", norm=True,
                    head_scale=1.0, seed=2004))
    return out


CASES = _table()
BY_NAME = {c["name"]: c for c in CASES}
LOGITS100 = [c["name"] for c in CASES if c["head_scale"] != 1.0]
NORM = [c["name"] for c in CASES if c["norm"]]


def num_params(dims):
    return sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))


def split_params(p, dims):
    """[(W [out, in], b [out])] views of a flat parameter vector in torch state_dict order."""
    out, off = [], 0
    for l in range(len(dims) - 1):
        i, o = dims[l], dims[l + 1]
        W = p[off: off + i * o].view(o, i)
        off += i * o
        out.append((W, p[off: off + o]))
        off += o
    return out


@functools.lru_cache(maxsize=None)
def inputs(case_name):
    """The case's fp32 / integer inputs on the CPU: p, X (a [N, D0] view of a wider table: row stride D0 + 3), Y (int32
    [N]), idx (int32 [n] or None), norm ((mean, std) with the zero std already replaced by 1, or None), raw_std."""
    c = BY_NAME[case_name]
    dims, n = c["dims"], c["n"]
    g = torch.Generator().manual_seed(c["seed"])
    parts = []
    for l in range(len(dims) - 1):
        i, o = dims[l], dims[l + 1]
        s = (2.0 if l < len(dims) - 2 else c["head_scale"]) / i ** 0.5
        parts += [(torch.rand(o, i, generator=g) * 2 - 1) * s, (torch.rand(o, generator=g) * 2 - 1) * s]
    p = torch.cat([t.reshape(-1) for t in parts]).float()
    N = max(n, 40) + 5
    table = torch.randn(N, dims[0] + 3, generator=g)
    norm = raw_std = None
    if c["norm"]:
        mean = torch.randn(dims[0], generator=g) * 3
        raw_std = torch.rand(dims[0], generator=g) * 4 + 0.5
        raw_std[min(1, dims[0] - 1)] = 0.0
        std = torch.where(raw_std == 0, torch.ones_like(raw_std), raw_std)
        table[:, : dims[0]] = table[:, : dims[0]] * std + mean  # raw-scale inputs
        norm = (mean.float(), std.float())
    X = table.float()[:, : dims[0]]
    Y = torch.randint(0, dims[-1], (N,), generator=g, dtype=torch.int32)
    idx = None
    if c["idx"] == "dup":
        idx = torch.randperm(N, generator=g)[:n].to(torch.int32)
        if n >= 4:  # duplicates: every fourth entry repeats its predecessor
            idx[3::4] = idx[2::4][: len(idx[3::4])]
    return dict(p=p, X=X, table=table.float(), Y=Y, idx=idx, norm=norm, raw_std=raw_std)


def rows_of(case_name):
    """(x fp32 [n, D0], y int64 [n]): the rows the launch visits, in order."""
    c, d = BY_NAME[case_name], inputs(case_name)
    sel = torch.arange(c["n"]) if d["idx"] is None else d["idx"].long()
    return d["X"][sel], d["Y"][sel].long()


def confusion(y, pred, C):
    return torch.bincount(y * C + pred, minlength=C * C).reshape(C, C)


def forward64(dims, p, x, norm=None):
    """fp64 forward with the derived logit bound: (logits [n, C], bound_z [n, C])."""
    a = x.double()
    e = torch.zeros_like(a)
    if norm is not None:
        a = (a - norm[0].double()) / norm[1].double()
        e = (2 * U + 4 * U * U) * a.abs()
    layers = split_params(p.double(), dims)
    for l, (W, b) in enumerate(layers):
        K = W.shape[1]
        z = a @ W.t() + b
        ez = (K + 2) * U * ((a.abs() + e) @ W.abs().t() + b.abs()) + e @ W.abs().t()
        if l < len(layers) - 1:
            a, e = torch.relu(z), ez
    return z, ez


def stats64(logits, bz, y, loss):
    """fp64 softmax, argmax, per-row loss and their bounds from fp64 logits and the logit bound."""
    n, C = logits.shape
    mx = logits.max(1, keepdim=True).values
    bmax = bz.max(1, keepdim=True).values
    probs = torch.softmax(logits, 1)
    d = bmax + U * ((mx - logits).max(1, keepdim=True).values + 2 * bmax)
    bp = probs * (torch.expm1(2 * d) + 16 * U) + TINY
    pred = logits.argmax(1)
    top2 = logits.topk(2, dim=1).values
    ambiguous = (top2[:, 0] - top2[:, 1]) < 2 * bmax[:, 0]
    zy = logits.gather(1, y[:, None])[:, 0]
    if loss == "ce":
        row_loss = torch.logsumexp(logits, 1) - zy
        bl = 2 * bmax[:, 0] + 16 * U + 4 * U * (mx[:, 0].abs() + zy.abs() + 2)
    else:
        dd = logits - torch.nn.functional.one_hot(y, C).double()
        row_loss = (dd * dd).mean(1)
        bl = (2 * dd.abs() * bz + bz * bz).mean(1) + 8 * U * row_loss + TINY
    return dict(probs=probs, bound_p=bp, pred=pred, ambiguous=ambiguous, row_loss=row_loss, bound_loss=bl)


@functools.lru_cache(maxsize=None)
def reference(case_name):
    """Everything a test compares against, fp64 on the CPU, computed once per case."""
    c, d = BY_NAME[case_name], inputs(case_name)
    x, y = rows_of(case_name)
    logits, bz = forward64(c["dims"], d["p"], x, d["norm"])
    out = dict(logits=logits, bound_z=bz, y=y)
    out.update(stats64(logits, bz, y, c["loss"]))
    return out


def expected_counts(ref, pred_seen, C):
    """(correct, confusion) the launch must report exactly: the fp64 prediction on the clear rows, the launch's own
    prediction on the ambiguous ones (whose argmax the bound does not decide)."""
    pred = torch.where(ref["ambiguous"], pred_seen.long(), ref["pred"])
    return int((pred == ref["y"]).sum()), confusion(ref["y"], pred, C)


# ----------------------------------------------------------------------------------------------- fp32 emulation
def _fma(acc, a, b):
    return (acc.double() + a.double() * b.double()).float()


def emulate(case_name, mutant=None):
    """The kernel's arithmetic in torch fp32, in its accumulation order: layer 0 a chain over k from the bias; the
    hidden x hidden layer the MFMA's chain from zero over k = 16 i + 4 q + t (t outer, q inner) plus the bias; the
    head eight interleaved partial chains, an xor tree, plus the bias.  Returns dict(logits, probs, pred, row_loss),
    fp32.  ``mutant``: "dropout" (p = 0.2 left on), "no_bias" (layer 0's), "relu_head", "softmax_no_max"."""
    c, d = BY_NAME[case_name], inputs(case_name)
    dims = c["dims"]
    x, y = rows_of(case_name)
    if d["norm"] is not None:
        x = (x - d["norm"][0]) / d["norm"][1]
    layers = split_params(d["p"], dims)
    L = len(layers)
    n = x.shape[0]
    g = torch.Generator().manual_seed(7)

    def hidden(z):
        z = torch.relu(z)
        if mutant == "dropout":
            keep = torch.rand(z.shape, generator=g) >= 0.2
            z = torch.where(keep, z * torch.tensor(1.25), torch.zeros(()))
        return z

    W, b = layers[0]
    z = (torch.zeros(n, W.shape[0]) if mutant == "no_bias" else b.expand(n, -1).clone())
    for k in range(dims[0]):
        z = _fma(z, W[:, k][None, :], x[:, k][:, None])
    a = hidden(z)
    if L == 3:
        W, b = layers[1]
        z = torch.zeros(n, W.shape[0])
        for i in range(dims[1] // 16):
            for t in range(4):
                for q in range(4):
                    k = 16 * i + 4 * q + t
                    z = _fma(z, a[:, k][:, None], W[:, k][None, :])
        a = hidden(z + b)
    W, b = layers[L - 1]
    part = []
    for s in range(8):
        acc = torch.zeros(n, W.shape[0])
        for k in range(s, W.shape[1], 8):
            acc = _fma(acc, W[:, k][None, :], a[:, k][:, None])
        part.append(acc)
    tree = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]))
    logits = tree + b
    if mutant == "relu_head":
        logits = torch.relu(logits)
    mx = logits.max(1, keepdim=True).values
    ex = torch.exp(logits if mutant == "softmax_no_max" else logits - mx)
    se = ex.sum(1, keepdim=True)
    probs = ex / se
    zy = logits.gather(1, y[:, None])[:, 0]
    if c["loss"] == "ce":
        row_loss = mx[:, 0] + torch.log(se[:, 0]) - zy
    else:
        dd = logits - torch.nn.functional.one_hot(y, dims[-1]).float()
        row_loss = (dd * dd).sum(1) / dims[-1]
    return dict(logits=logits, probs=probs, pred=logits.argmax(1), row_loss=row_loss)


def inside(got, ref):
    """The per-element checks of a result against the reference: dict of booleans."""
    lo = (got["logits"].double() - ref["logits"]).abs() <= ref["bound_z"]
    finite = bool(torch.isfinite(got["probs"]).all())
    pr = finite and bool(((got["probs"].double() - ref["probs"]).abs() <= ref["bound_p"]).all())
    clear = ~ref["ambiguous"]
    return dict(logits=bool(lo.all()), probs=pr, finite=finite,
                pred=bool((got["pred"][clear] == ref["pred"][clear]).all()),
                row_loss=bool(((got["row_loss"].double() - ref["row_loss"]).abs() <= ref["bound_loss"]).all()))
