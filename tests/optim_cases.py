"""AdamW and SGD (momentum, dampening, Nesterov) in the batch-tiled MLP trainer's fold (csrc/mlp_tile.hip,
MlpArgs::opt_kind) and the flat SGD step (csrc/optim.hip dct_sgd_flat_step): the cases the GPU tests run, their fp64
reference, the bound derived from the kernels' fp32 operations, and the wrong implementations the bound must reject.

torch's formulas (maximize=False, amsgrad=False), with g the step's gradient and lr_t the step's rate (the lr table's
entry when one is bound, the scalar otherwise):

    SGD    g1 = g + wd p
           momentum mu != 0:  buf' = g1 on the first step (torch has no buffer yet; what the buffer held is ignored),
                              else mu buf + (1 - damp) g1;   d = g1 + mu buf' (Nesterov) or buf'
           mu == 0:           d = g1
           p' = p - lr_t d
    AdamW  p1 = p (1 - lr_t wd);  m' = b1 m + (1 - b1) g;  v' = b2 v + (1 - b2) g^2
           p' = p1 - (lr_t / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps),   t = steps taken + 1

``CASES``: accum_cases.CASES' shapes (dims, B) with wloss_cases' inputs.  ``VARIANTS``: the five hyper-parameter sets,
all at lr_t = 0.01.  ``STEP_COUNTS``: 0 (the first-step rule; SGD's buffer is pre-filled with garbage, NaNs included)
and 3 (random non-zero m / v).  ``LR_BASE`` is the scalar rate handed to a launch that also binds a table holding
0.01: a kernel that reads the scalar anywhere is off by a factor 3 there.

``reference(p, g, m, v, hp, taken, mutant=None)``: fp64 from fp32 inputs.  As in tests/wide_step_cases.py the
hyper-parameters are rounded to fp32 first (the kernels get them as floats; (1 - 0.999) in fp32 is 6e-5 away from the
double's), and tests/test_optim_cases_cpu.py steps torch's own optimizers in fp64 with those same values.

Bounds, u = 2^-24 per fp32 rounding, each rounding relative to an intermediate that the sum of the absolute values of
its terms bounds (a fused multiply-add rounds once where the count below has two: never more).  Nothing is measured.
  SGD    g1: product and sum when wd != 0, Ng = 2 (else 0) roundings of Tg = |g| + wd |p|.
         buf' (not the first step): mu buf (1), 1 - damp (1: not exact in fp32), its product with g1 (1), the sum (1);
                 the deeper term carries Ng + 2, the sum one more: (Ng + 3) u Tb, Tb = mu |buf| + (1 - damp) Tg.
                 First step: buf' = g1, Ng u Tg.
         d:      Nesterov: g1's and mu buf's errors, the product and the sum: b_g + mu b_buf + 2 u Td, Td = Tg + mu Tb;
                 otherwise buf's (or g1's).
         p':     lr_t b_d + u lr_t Td (product) + u (|p| + lr_t Td) (difference).
  AdamW  the device bias corrections 1 - exp2(t log2f(b)): the argument a = t log2 b carries 3 u |a| (log2f, the
         product), v_exp_f32 is good to 1 ulp = 2 u, so b^t is off by at most b^t (2 + 3 |a|) u and the correction by
         c(b, t) = u ((2 + 3 |a|) b^t / (1 - b^t) + 1) relative.  step_size = lr_t / bc1: c(b1, t) + u;
         rbc2 = v_rsq_f32(bc2), 1 ulp: c(b2, t) + 2 u (c / 2 would do).
         m': 3 u Tm, Tm = b1 |m| + (1 - b1) |g| ((1 - b1) and (1 - b2) are exact in fp32 for b in [0.5, 1]);
         v': 4 u Tv.  D = v_sqrt_f32(v') rbc2 + eps: v's bound through the concave sqrt, then 1 ulp (2 u), the product,
         the sum and rbc2's error: eD = rbc2 (sqrt(v') - sqrt(v' - bv)) + (4 u + c2) D.
         update = step_size m' v_rcp_f32(D): step_size bm / D + |update| (4 u + eD / (D - eD) + c1)  (two products,
         the 1-ulp reciprocal).  p1 = p (1 - lr_t wd): lr_t wd (1), the difference (1, relative to ~1), the product
         (1): u |p| (2 + 2 lr_t wd).  The final difference: u (|p1| + |update|).

A plain module, not a conftest: the tests import it."""
import math
from collections import namedtuple

import numpy as np
import torch

import accum_cases as ac
import infer_cases as ic
import wloss_cases as wc

U = 2.0 ** -24
TINY = 2.0 ** -149
SECOND_ORDER = 1.0 + 2.0 ** -18  # as tests/wide_step_cases.py: products of the <= 32 roundings counted

CASES = [(dims, B) for dims, B, _ in ac.CASES]  # [5,64,2] at 4 and 40, [7,48,32,3] at 65, [32,128,128,4] at 17
Hyper = namedtuple("Hyper", "kind lr momentum dampening nesterov wd b1 b2 eps")
LR, LR_BASE = 0.01, 0.03
VARIANTS = {
    "sgd": Hyper("sgd", LR, 0.0, 0.0, False, 0.0, 0.9, 0.999, 1e-8),
    "sgd_m": Hyper("sgd", LR, 0.9, 0.0, False, 0.0, 0.9, 0.999, 1e-8),
    "sgd_mdw": Hyper("sgd", LR, 0.9, 0.1, False, 0.05, 0.9, 0.999, 1e-8),
    "sgd_nest": Hyper("sgd", LR, 0.9, 0.0, True, 0.05, 0.9, 0.999, 1e-8),
    "adamw": Hyper("adamw", LR, 0.0, 0.0, False, 0.05, 0.9, 0.999, 1e-8),
}
STEP_COUNTS = (0, 3)
# first_dampened: the first step's buffer is (1 - damp) g1; first_reads_m: the first step runs the recurrence on what
# the buffer held; nesterov_ignored: d = buf'; nesterov_old_buf: d = g1 + mu buf (before its update); sgd_decoupled:
# p (1 - lr wd) instead of g + wd p; adamw_coupled: g + wd p instead of the decay; adamw_base_rate: the decay uses the
# scalar rate, not the table's; dampening_ignored: buf' = mu buf + g1; momentum_on_p: p' = p - lr g1 - mu buf'
MUTANTS = ["first_dampened", "first_reads_m", "nesterov_ignored", "nesterov_old_buf", "sgd_decoupled",
           "adamw_coupled", "adamw_base_rate", "dampening_ignored", "momentum_on_p"]


def f32(x):
    return float(np.float32(x))


def case_id(case):
    dims, B = case
    return ic.name(dims) + f"-b{B}"


def kernel_args(hp):
    """The optimizer keywords of FusedMLPKernel.train for a variant (without lr)."""
    if hp.kind == "sgd":
        return dict(optimizer="sgd", momentum=hp.momentum, dampening=hp.dampening, nesterov=hp.nesterov,
                    weight_decay=hp.wd)
    return dict(optimizer="adamw", betas=(hp.b1, hp.b2), eps=hp.eps, weight_decay=hp.wd)


def torch_optimizer(params, hp, lr=None, dtype_exact=True):
    """torch's own optimizer of a variant; ``dtype_exact``: with the hyper-parameters rounded to fp32 (the values the
    kernels get), for the fp64 comparison."""
    r = f32 if dtype_exact else float
    lr = hp.lr if lr is None else lr
    if hp.kind == "sgd":
        return torch.optim.SGD(params, lr=r(lr), momentum=r(hp.momentum), dampening=r(hp.dampening),
                               nesterov=hp.nesterov, weight_decay=r(hp.wd))
    return torch.optim.AdamW(params, lr=r(lr), betas=(r(hp.b1), r(hp.b2)), eps=r(hp.eps), weight_decay=r(hp.wd))


def state(case, hp, taken):
    """(p, m, v) fp32 on the CPU before the step: p the case's parameters (wloss_cases.inputs).  taken == 0: SGD's
    buffer holds garbage (large values, a NaN every 7th word) that the first step must ignore, AdamW's moments are
    torch's zeros; taken > 0: random non-zero m (and v > 0)."""
    dims, B = case
    p = wc.inputs((dims, B))["p"].clone()
    g = torch.Generator().manual_seed(97 * B + dims[0] + 7 * taken)
    n = p.numel()
    if taken == 0:
        if hp.kind == "sgd":
            m = torch.randn(n, generator=g) * 1e3
            m[::7] = float("nan")
        else:
            m = torch.zeros(n)
        v = torch.zeros(n)
    else:
        m = torch.randn(n, generator=g) * 0.05
        v = torch.rand(n, generator=g) * 1e-3 + 1e-7
    return p, m.float(), v.float()


def cpu_gradient(case):
    """An fp32 gradient vector for the tests without a GPU: torch autograd's, in fp32, of the mean cross-entropy over
    the case's first batch."""
    dims, B = case
    d = wc.inputs((dims, B))
    p = d["p"].clone().requires_grad_()
    sel = d["idx"][:B].long()
    h = d["X"][sel]
    layers = ic.split_params(p, dims)
    for li, (W, b) in enumerate(layers):
        h = h @ W.t() + b
        if li < len(layers) - 1:
            h = torch.relu(h)
    torch.nn.functional.cross_entropy(h, d["Y"][sel].long()).backward()
    return p.grad.detach().float()


def _c_bc(b, t):
    """Relative error granted to the device bias correction 1 - exp2(t log2f(b)) (module docstring)."""
    a = abs(t * math.log2(b))
    bt = b ** t
    return U * ((2.0 + 3.0 * a) * bt / (1.0 - bt) + 1.0)


Ref = namedtuple("Ref", "p m v p_bound m_bound v_bound")


def reference(p, g, m, v, hp, taken, mutant=None, lr_base=None):
    """One step in fp64 from fp32 inputs after ``taken`` steps: Ref(p, m, v, and their absolute error bounds for an
    fp32 evaluation in the kernels' operation order); v is None for SGD, m too without momentum.  ``lr_base``: the
    scalar rate of a launch that reads the step's rate hp.lr from a table (only the adamw_base_rate mutant uses it)."""
    lr, mu, damp, wd, b1, b2, eps = (f32(x) for x in (hp.lr, hp.momentum, hp.dampening, hp.wd, hp.b1, hp.b2, hp.eps))
    p0, g0, m0 = p.double(), g.double(), m.double()
    first = taken == 0
    if hp.kind == "sgd":
        assert damp <= 0.5  # (1 - damp) counted as one rounding of a value >= 0.5
        omd = 1.0 - damp
        decoupled = mutant == "sgd_decoupled"
        g1 = g0 if decoupled else g0 + wd * p0
        pd = p0 * (1.0 - lr * wd) if decoupled else p0
        ng = 2.0 if wd else 0.0
        Tg = g0.abs() + wd * p0.abs()
        bg = ng * U * Tg
        if mu == 0.0:
            d, bd, Td, m1, bm = g1, bg, Tg, None, None
        else:
            if first and mutant != "first_reads_m":
                m1 = (omd if mutant == "first_dampened" else 1.0) * g1
                bm, Tb = bg, Tg
            else:
                m1 = mu * m0 + (1.0 if mutant == "dampening_ignored" else omd) * g1
                Tb = mu * m0.abs() + omd * Tg
                bm = (ng + 3.0) * U * Tb
            if hp.nesterov and mutant != "nesterov_ignored":
                d = g1 + mu * (m0 if mutant == "nesterov_old_buf" else m1)
                Td = Tg + mu * Tb
                bd = bg + mu * bm + 2.0 * U * Td
            else:
                d, bd, Td = m1, bm, Tb
        p1 = pd - lr * g1 - mu * m1 if (mutant == "momentum_on_p" and m1 is not None) else pd - lr * d
        bp = (lr * bd + U * lr * Td + U * (p0.abs() + lr * Td)) * SECOND_ORDER + 2 * TINY
        return Ref(p1, m1, None, bp, None if bm is None else bm * SECOND_ORDER + 2 * TINY, None)
    v0 = v.double()
    t = taken + 1
    omb1, omb2 = 1.0 - b1, 1.0 - b2  # exact in fp32 too (Sterbenz: b in [0.5, 1])
    assert b1 >= 0.5 and b2 >= 0.5
    lr_decay = f32(lr_base) if (mutant == "adamw_base_rate" and lr_base is not None) else lr
    if mutant == "adamw_coupled":
        g1, pd = g0 + wd * p0, p0
    else:
        g1, pd = g0, p0 * (1.0 - lr_decay * wd)
    step_size, rbc2 = lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)
    c1, c2 = _c_bc(b1, t) + U, _c_bc(b2, t) + 2.0 * U
    m1 = b1 * m0 + omb1 * g1
    v1 = b2 * v0 + omb2 * g1 * g1
    bm = 3.0 * U * (b1 * m0.abs() + omb1 * g0.abs()) * SECOND_ORDER + 6 * TINY
    bv = 4.0 * U * (b2 * v0 + omb2 * g0 * g0) * SECOND_ORDER + 8 * TINY
    sq = v1.sqrt()
    D = sq * rbc2 + eps
    eD = rbc2 * (sq - (v1 - bv).clamp_min(0).sqrt()) + (4.0 * U + c2) * D
    upd = step_size * m1 / D
    bu = step_size * bm / D + upd.abs() * (4.0 * U + eD / (D - eD) + c1) * SECOND_ORDER
    p1 = pd - upd
    bp = bu + U * p0.abs() * (2.0 + 2.0 * lr * wd) + U * (pd.abs() + upd.abs()) + 2 * TINY
    return Ref(p1, m1, v1, bp, bm, bv)


def emulate_fp32(p, g, m, v, hp, taken):
    """The kernels' operation order in numpy fp32, every operation rounded on its own (no fused multiply-add;
    correctly rounded sqrt and reciprocal standing in for the 1-ulp hardware ones): (p, m, v) as fp32 tensors."""
    f = np.float32
    lr, mu, damp, wd, b1, b2, eps = (f(x) for x in (hp.lr, hp.momentum, hp.dampening, hp.wd, hp.b1, hp.b2, hp.eps))
    P, G, M = p.numpy().astype(f), g.numpy().astype(f), m.numpy().astype(f)
    with np.errstate(invalid="ignore"):
        if hp.kind == "sgd":
            G = G + wd * P
            if mu != 0:
                Bn = G if taken == 0 else mu * M + (f(1) - damp) * G
                D = G + mu * Bn if hp.nesterov else Bn
                return torch.from_numpy(P - lr * D), torch.from_numpy(Bn.astype(f)), None
            return torch.from_numpy(P - lr * G), None, None
        V = v.numpy().astype(f)
        t = f(taken + 1)
        bc1 = f(1) - np.exp2(t * np.log2(b1)).astype(f)
        bc2 = f(1) - np.exp2(t * np.log2(b2)).astype(f)
        step_size, rbc2 = lr / bc1, f(1) / np.sqrt(bc2)
        P = P * (f(1) - lr * wd)
        M = b1 * M + (f(1) - b1) * G
        V = b2 * V + (f(1) - b2) * G * G
        den = np.sqrt(V) * rbc2 + eps
        P = P - step_size * M * (f(1) / den)
    return torch.from_numpy(P.astype(f)), torch.from_numpy(M.astype(f)), torch.from_numpy(V.astype(f))


def inside(got, ref):
    """(p, m, v) of an fp32 evaluation against a Ref: every element within its bound (a NaN is outside; a buffer the
    optimizer does not have is not compared)."""
    ok = True
    for x, want, bound in zip(got, (ref.p, ref.m, ref.v), (ref.p_bound, ref.m_bound, ref.v_bound)):
        if want is None:
            continue
        ok = ok and bool(((x.double() - want).abs() <= bound).all())
    return ok


def excess(got, ref):
    """Worst |error| / bound over p, m, v (<= 1 passes; nan stays nan), for printing."""
    worst = 0.0
    for x, want, bound in zip(got, (ref.p, ref.m, ref.v), (ref.p_bound, ref.m_bound, ref.v_bound)):
        if want is not None:
            r = ((x.double() - want).abs() / bound).max()
            worst = float(r) if math.isnan(float(r)) else max(worst, float(r))
    return worst
