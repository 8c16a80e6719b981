"""The classifier-head launchers as tables of cases with fp64 references and derived bounds: dct_skinny_fwd / _dx / _dw
and the fused dct_skinny_head (csrc/skinny.hip), dct_loss_fwd_bwd[_ex] (csrc/nn_kernels.hip loss_kernel).
tests/test_skinny_cases_cpu.py runs a torch fp32 / bf16 emulation (and mutants) against the bounds and checks that the
head table reaches every instantiation of the launcher's switch; tests/test_skinny_kernels_gpu.py launches them.

Conventions (wide_step_cases / tt_cases): u = 2^-24 per fp32 rounding, BF = 2^-8 per bf16 rounding, HW = 2 u per
hardware transcendental (__expf, __logf, 1.f / s).  A product of two bf16 values is exact in fp32.  A sum whose terms
each pass through at most d additions (in a thread, across a wave, across the waves of a block, then one atomic per
block) is off by at most d u (sum |terms| + |initial value|): the `depth` arguments below count d from the launch
geometry.

Hidden roundings - the fused head rounds its logits z and its dz to bf16 "like the unfused bf16 logits" without ever
storing them - are charged as error terms (BF |z|, BF |dz|), never replayed, so a rounding tie cannot flip a verdict.
That dz IS rounded shows in one place: with one row and db starting at zero, db[c] is dz[c] itself and must be a bf16
value (head_check's "dz_is_bf16").

A plain module, not a conftest: the tests import it."""
import functools
import math

import torch

from gemm_cases import MIN_BF16
from tt_cases import BF, HW, bf, ratio
from wide_step_cases import SECOND_ORDER, TINY, U, f32, fwd_bound, gemm_ref  # f32: a scalar argument as launched


def ct_of(C):
    """The class-count template argument: C rounded up to 1, 2, 4, 8."""
    return 1 if C == 1 else 2 if C == 2 else 4 if C <= 4 else 8


# ------------------------------------------------------------------------------------------------ loss chain
def first_argmax(z):
    """The lowest index holding the row maximum: both kernel paths scan upwards with a strict >."""
    m = z.max(-1, keepdim=True).values
    return ((z == m).int().cumsum(-1) == 0).sum(-1)


def loss_chain(z, e_z, y, kind, grad_scale):
    """Row losses and dL/dz * grad_scale in fp64 of logits z [B][C] known to within e_z, with bounds for the kernels'
    fp32 evaluation (skinny_head_kernel and loss_kernel use the same formulas).

    CE: m = max z (|max a - max b| <= max |a - b|), d = z - m, e = __expf(d) (the argument's error through exp, the
    product with log2 e and v_exp_f32: expm1(2 u |d|) + HW relative), s = sum e (C <= 16 additions of positive terms),
    loss = m + __logf(s) - z_y, dz = (e / s - onehot) grad_scale (1 / s: HW; two products; the subtraction).
    MSE: d = z - onehot, loss = sum d^2 / C, dz = 2 d grad_scale / C (three roundings)."""
    B, C = z.shape
    grad_scale = f32(grad_scale)
    onehot = torch.zeros(B, C, dtype=torch.float64)
    onehot[torch.arange(B), y] = 1.0
    if kind == 0:
        m = z.max(-1, keepdim=True).values
        e_m = e_z.max(-1, keepdim=True).values
        d = z - m
        e_d = e_z + e_m + U * d.abs()
        ek = torch.exp(d)
        rk = torch.expm1(e_d) + torch.expm1(2 * U * d.abs()) + HW
        se = ek.sum(-1, keepdim=True)
        r_se = (ek * rk).sum(-1, keepdim=True) / se + 16 * U
        logse = torch.log(se)
        e_logse = -torch.log1p(-r_se.clamp_max(0.5)) + HW * logse.abs().clamp_min(1.0) + U * logse.abs()
        zy = (z * onehot).sum(-1, keepdim=True)
        lb = m + logse - zy
        e_lb = e_m + (e_z * onehot).sum(-1, keepdim=True) + e_logse + U * (m + logse).abs() + U * lb.abs()
        soft = ek / se
        e_soft = soft * (rk + r_se + HW + U) * SECOND_ORDER
        g = soft - onehot
        dz = g * grad_scale
        e_dz = (e_soft + U * g.abs()) * abs(grad_scale) + U * dz.abs()
        return lb.reshape(B), e_lb.reshape(B) + TINY, dz, e_dz + TINY
    d = z - onehot
    e_d = e_z + U * d.abs()
    sq = (d * d).sum(-1)
    lb = sq / C
    e_lb = ((2 * d.abs() * e_d + e_d * e_d).sum(-1) + (C + 1) * U * sq) / C + 2 * U * lb
    dz = 2.0 * d * grad_scale / C
    e_dz = 2.0 * abs(grad_scale) / C * e_d + 3 * U * dz.abs()
    return lb, e_lb + TINY, dz, e_dz + TINY


def sum_bound(e_terms_sum, abs_sum, init, ref, depth):
    """A reduction of terms known to e each into ``init``: their errors, depth u of the magnitudes, the result's own."""
    return (e_terms_sum + depth * U * (abs_sum + init.abs()) + U * ref.abs()) * SECOND_ORDER + TINY


def _loss32(z, y, kind, grad_scale, C, mutant=None):
    """The same chain op by op in torch fp32."""
    B = z.shape[0]
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    onehot = torch.zeros(B, C)
    onehot[torch.arange(B), y] = 1.0
    gs = f(1.0) if mutant == "ce_no_grad_scale" and kind == 0 else f(grad_scale)
    if kind == 0:
        m = z.max(-1, keepdim=True).values
        ek = torch.exp(z - m)
        se = ek.sum(-1, keepdim=True)
        rl = (m + torch.log(se) - (z * onehot).sum(-1, keepdim=True)).reshape(B)
        dz = (ek * (1.0 / se) - onehot) * gs
    else:
        d = z - onehot
        div = f(1.0) if mutant == "mse_no_1_over_c" else f(float(C))
        rl = (d * d).sum(-1) / div
        dz = 2.0 * d * gs / div
    return rl, dz


# ------------------------------------------------------------------------------------------------ skinny fwd / dx / dw
SK_CS, SK_KS, SK_BS = (1, 2, 3, 4, 5, 8), (8, 264, 520, 1024), (1, 3, 65, 777)
SK_DX_GRID_STRIDE = (4100, 2048, 2)  # B K / 8 = 1049600 > 4096 * 256 threads: 1024 of them take a second element


def sk_cases():
    """(B, K, C): every C with every K and every B at least once, B and K cycling against each other."""
    out = []
    for ci, C in enumerate(SK_CS):
        for ki, K in enumerate(SK_KS):
            out.append((SK_BS[(ci + ki) % 4], K, C))
            out.append((SK_BS[(ci + ki + 2) % 4], K, C))
    return out


def dw_geometry(B, K):
    """(column blocks, row splits, rows_per) of dct_skinny_dw."""
    kb = -(-K // 512)
    splits = max(1, min(-(-256 // kb), -(-B // 64)))
    rows_per = -(-B // splits)
    return kb, -(-B // rows_per), rows_per


@functools.lru_cache(maxsize=4)
def sk_problem(B, K, C):
    g = torch.Generator().manual_seed(100000 * C + 10 * K + B)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = r(B, K)
    x[:, ::3] = torch.relu(x[:, ::3])          # a ReLU output in a third of the columns: exact zeros for the dX mask
    x = bf(x)
    if B * K > 8:
        x.view(-1)[1], x.view(-1)[2] = -0.0, MIN_BF16
    return dict(x=x, w=bf(r(C, K) / math.sqrt(K)), bias=r(C) * 0.5, dz=bf(r(B, C) / max(B, 1) ** 0.5),
                dw0=r(C, K), db0=r(C) * 2.0)


def sk_fwd_expect(p, with_bias=True):
    """Y = bf16(x w^T + bias): fwd_bound plus the bias addition's own rounding."""
    z, ap = gemm_ref(p["x"], p["w"].t())
    if with_bias:
        z = z + p["bias"].double()
    return z, fwd_bound(z, ap, p["x"].shape[1]) + 2 * U * z.abs()


def sk_dx_expect(p, masked):
    """dX = bf16(dz w) over C exact products, masked to exact zeros where aux <= 0."""
    z, ap = gemm_ref(p["dz"], p["w"])
    C = p["w"].shape[0]
    e = (C * U * ap) * SECOND_ORDER * (1 + BF) + BF * z.abs() + TINY
    if masked:
        keep = p["x"].double() > 0
        z, e = torch.where(keep, z, torch.zeros_like(z)), torch.where(keep, e, torch.full_like(e, TINY))
    return z, e


def sk_dw_expect(p):
    """dW += dz^T x, db += colsum dz: exact products; a term passes its thread's ceil(rows_per / 4) additions, the
    4-wave fold and one atomic per row split."""
    B, K = p["x"].shape
    _, ny, rows_per = dw_geometry(B, K)
    depth = -(-rows_per // 4) + 4 + ny + 1
    z, ap = gemm_ref(p["dz"].t(), p["x"])
    dw = p["dw0"].double() + z
    dzs = p["dz"].double()
    db = p["db0"].double() + dzs.sum(0)
    return dict(dW=(dw, sum_bound(0.0, ap, p["dw0"].double(), dw, depth)),
                db=(db, sum_bound(0.0, dzs.abs().sum(0), p["db0"].double(), db, depth)))


def sk_emulate(p, what, mutant=None, masked=True, with_bias=True):
    x, w, dz = p["x"].float(), p["w"].float(), p["dz"].float()
    C = w.shape[0]
    if mutant == "last_class_weights_for_c_minus_2" and C >= 2:
        w = w.clone()
        w[C - 2] = w[C - 1]
    if what == "fwd":
        return bf(x @ w.t() + (p["bias"] if with_bias else 0.0))
    if what == "dx":
        o = dz @ w
        return bf(torch.where(x > 0, o, torch.zeros_like(o)) if masked else o)
    kb = dw_geometry(*x.shape)[0]
    return dict(dW=p["dw0"] + dz.t() @ x,
                db=p["db0"] + dz.sum(0) * (kb if mutant == "db_once_per_column_block" else 1))


# ------------------------------------------------------------------------------------------------ fused head
HEAD_INSTANCES = sorted({(ct, nj, w) for ct in (1, 2) for nj in (1, 2) for w in (4, 8)} |
                        {(ct, nj, 4) for ct in (1, 2) for nj in (3, 4)} | {(4, 1, 4), (4, 2, 4), (8, 1, 4)})
HEAD_SUPPORT = [(512, 1), (2048, 2), (2560, 2), (1536, 3), (1024, 4), (1024, 5), (512, 8), (512, 9), (520, 2), (256, 1),
                (0, 1), (512, 0), (1024, 8)]


def head_supported(K, C):
    """The documented rule: K a multiple of 512 with C <= 2 and K <= 2048, C <= 4 and K <= 1024, or C <= 8 and K = 512."""
    if C < 1 or K < 512 or K % 512:
        return False
    return (C <= 2 and K <= 2048) or (C <= 4 and K <= 1024) or (C <= 8 and K == 512)


def head_kernel(B, K, C):
    """(CT, NJ, NWV) of the skinny_head_kernel instantiation the launcher picks."""
    nwv = 8 if C <= 2 and K <= 1024 and B >= 128 * 32 else 4
    return ct_of(C), K // 512, nwv


# (B, K, C, relu_mask, nulls, grad_scale, loss_scale); both loss kinds run on each
def head_cases():
    out = []
    nulls = [(), ("dH",), ("db",), ("loss_sum",), ("bias",), ("dH", "db", "loss_sum", "bias")]
    bs = (1, 5, 17, 130)
    shapes = ([(C, K) for C in (1, 2) for K in (512, 1024, 1536, 2048)] + [(C, K) for C in (3, 4) for K in (512, 1024)] +
              [(5, 512), (8, 512)])
    for i, (C, K) in enumerate(shapes):
        B = bs[i % 4]
        out.append((B, K, C, i % 2, nulls[i % 6], 1.0 / 3.0, 1.0 / B))
    for i, (C, K) in enumerate([(1, 512), (1, 1024), (2, 512), (2, 1024)]):
        out.append((4099, K, C, (i + 1) % 2, nulls[i % 2], 1.0 / 4099, 1.0 / 3.0))
    # one row and everything set: db is dz itself (the bf16 check); every B once more on the smallest shape
    out += [(1, 512, 2, 1, (), 1.0 / 3.0, 1.0 / 3.0), (1, 512, 8, 0, (), 1.0 / 3.0, 1.0), (1, 1024, 4, 0, (), 1.0 / 3.0, 1.0)]
    out += [(B, 512, 2, 1, (), 1.0 / B, 1.0 / 3.0) for B in (5, 17, 130)]
    return out


HEAD_REJECTED = [("K = 520", dict(K=520)), ("C = 3 with K = 1536", dict(K=1536, C=3)), ("C = 9", dict(C=9)),
                 ("null dW", dict(null="dW")), ("null labels", dict(null="labels")), ("null H", dict(null="H")),
                 ("H not 16-byte aligned", dict(shift="H")), ("dH not 16-byte aligned", dict(shift="dH"))]


@functools.lru_cache(maxsize=4)
def head_problem(B, K, C):
    g = torch.Generator().manual_seed(7 + 100000 * C + 10 * K + B)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    h = bf(torch.relu(r(B, K)))                       # a ReLU output: half exact zeros for relu_mask
    if B * K > 8:
        h.view(-1)[1], h.view(-1)[2] = -0.0, MIN_BF16
    y = (torch.arange(B) + (C - 1)) % C               # every class, C - 1 first
    one = B == 1
    return dict(h=h, w=bf(r(C, K) * 2.0 / math.sqrt(K)), bias=r(C) * 0.5, y=y.to(torch.int32),
                dw0=torch.zeros(C, K) if one else r(C, K), db0=torch.zeros(C) if one else r(C) * 2.0,
                loss0=torch.tensor([0.0 if one else 1.5]))


def head_expect(p, kind, relu_mask, grad_scale, loss_scale, with_bias=True):
    """z = H W^T + bias in fp32 then the hidden bf16 rounding: K u sum|h||w| + 2 u |z| + BF |z|.  loss_chain on it;
    dz's hidden rounding BF |dz|.  dH = bf16(dz W): C exact products of the rounded dz with W.  dW, db, loss: a term
    passes its wave's 4 rows, the fold of up to 8 waves and one atomic per block."""
    h, w = p["h"], p["w"]
    B, K = h.shape
    C = w.shape[0]
    nwv = head_kernel(B, K, C)[2]
    nb = -(-B // (4 * nwv))
    depth = 4 + 8 + nb + 1
    z, ap = gemm_ref(h, w.t())
    if with_bias:
        z = z + p["bias"].double()
    e_z = (K * U * ap + 2 * U * z.abs()) * SECOND_ORDER + BF * z.abs() + TINY
    lb, e_lb, dz, e_dz = loss_chain(z, e_z, p["y"].long(), kind, grad_scale)
    e_dz = e_dz * (1 + BF) + BF * dz.abs()
    W, hd = w.double(), h.double()
    dh = dz @ W
    e_dh = (e_dz @ W.abs() + C * U * (dz.abs() + e_dz) @ W.abs()) * (1 + BF) + BF * dh.abs() + TINY
    if relu_mask:
        keep = hd > 0
        dh, e_dh = torch.where(keep, dh, torch.zeros_like(dh)), torch.where(keep, e_dh, torch.full_like(e_dh, TINY))
    dw0, db0, l0 = p["dw0"].double(), p["db0"].double(), p["loss0"].double()
    loss_scale = f32(loss_scale)
    dw = dw0 + dz.t() @ hd
    db = db0 + dz.sum(0)
    loss = l0 + loss_scale * lb.sum()
    ls = abs(loss_scale)
    return dict(dH=(dh, e_dh),
                dW=(dw, sum_bound(e_dz.t() @ hd.abs(), (dz.abs() + e_dz).t() @ hd.abs(), dw0, dw, depth)),
                db=(db, sum_bound(e_dz.sum(0), (dz.abs() + e_dz).sum(0), db0, db, depth)),
                loss=(loss, sum_bound(ls * e_lb.sum() + 2 * U * ls * lb.abs().sum(), ls * lb.abs().sum(), l0, loss,
                                      depth)))


def head_check(got, p, kind, relu_mask, grad_scale, loss_scale, with_bias=True):
    """{tensor: worst error / bound} of the outputs present in ``got`` (dH, dW, db, loss), plus "dz_is_bf16" for a
    one-row problem whose db started at zero."""
    ref = head_expect(p, kind, relu_mask, grad_scale, loss_scale, with_bias)
    out = {k: ratio(got[k], *ref[k]) for k in ref if got.get(k) is not None}
    if p["h"].shape[0] == 1 and got.get("db") is not None:
        db = got["db"].float()
        out["dz_is_bf16"] = 0.0 if bool((bf(db).float() == db).all()) else float("inf")
    return out


HEAD_MUTANTS = ["last_class_weights_for_c_minus_2", "dz_not_rounded", "mse_no_1_over_c", "ce_no_grad_scale",
                "loss_scale_ignored"]


def head_emulate(p, kind, relu_mask, grad_scale, loss_scale, with_bias=True, mutant=None):
    h, w = p["h"].float(), p["w"].float()
    C = w.shape[0]
    wz = w
    if mutant == "last_class_weights_for_c_minus_2" and C >= 2:
        wz = w.clone()
        wz[C - 2] = w[C - 1]
    z = bf(h @ wz.t() + (p["bias"] if with_bias else 0.0)).float()
    rl, dz = _loss32(z, p["y"].long(), kind, grad_scale, C, mutant)
    if mutant != "dz_not_rounded":
        dz = bf(dz).float()
    o = dz @ w
    ls = 1.0 if mutant == "loss_scale_ignored" else loss_scale
    return dict(dH=bf(torch.where(h > 0, o, torch.zeros_like(o)) if relu_mask else o), dW=p["dw0"] + dz.t() @ h,
                db=p["db0"] + dz.sum(0), loss=p["loss0"] + rl.sum() * torch.tensor(ls, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ loss kernel
LOSS_CS, LOSS_MS = (1, 2, 3, 8, 9, 16), (1, 1000)
LOSS_BIG_M = 262144 + 5  # 1024 workgroups of 256 rows, then 5 rows in a second grid-stride pass
LOSS_BIG = [(2, 1, 0), (9, 0, 1), (16, 1, 1), (8, 0, 0)]  # (C, bf16 logits, loss kind) at LOSS_BIG_M
LOSS_NULLS = [(), ("dlogits",), ("loss_sum",), ("correct_sum",)]


def loss_path(C):
    return "registers (C <= 8)" if C <= 8 else "generic loop (C > 8)"


@functools.lru_cache(maxsize=2)
def loss_problem(M, C, lbf16):
    """Logits with row scales 1, 5 and 30 (clipped to +-30), exact ties for the maximum in every third row (between
    the first maximum and a later class, and in every ninth row a tie of ALL classes), labels over every class."""
    g = torch.Generator().manual_seed(31 * M + 7 * C + lbf16)
    z = torch.randn(M, C, generator=g) * torch.tensor([1.0, 5.0, 30.0])[torch.arange(M) % 3].reshape(M, 1)
    z = z.clamp(-30.0, 30.0)
    if lbf16:
        z = bf(z).float()
    rows = torch.arange(0, M, 3)
    if C > 1:
        m = z[rows].max(-1).values
        z[rows, (first_argmax(z[rows]) + 1 + rows) % C] = m
        z[torch.arange(0, M, 9)] = z[torch.arange(0, M, 9), :1]
    y = ((torch.arange(M) * 7 + C - 1) % C).to(torch.int32)
    return dict(z=bf(z) if lbf16 else z, y=y, loss0=torch.tensor([2.5]), correct0=torch.tensor([3.0]))


def loss_geometry(M):
    nb = max(1, min(1024, -(-M // 256)))
    return nb, -(-M // (nb * 256))


def loss_expect(p, kind, grad_scale, loss_scale, lbf16):
    """The logits are exact inputs.  dlogits: loss_chain's bound, plus the bf16 rounding of the stored value when the
    logits are bf16.  loss_sum: a row's loss passes its thread's rows, 6 wave steps, 4 waves, the scaling and one
    atomic per block.  correct_sum counts rows in fp32 integers: exact."""
    z = p["z"].double()
    M, C = z.shape
    nb, rpt = loss_geometry(M)
    lb, e_lb, dz, e_dz = loss_chain(z, torch.zeros_like(z), p["y"].long(), kind, grad_scale)
    if lbf16:
        e_dz = e_dz * (1 + BF) + BF * dz.abs()
    loss_scale = f32(loss_scale)
    ls = abs(loss_scale)
    l0 = p["loss0"].double()
    loss = l0 + loss_scale * lb.sum()
    correct = p["correct0"].double() + (first_argmax(z) == p["y"].long()).sum()
    return dict(dlogits=(dz, e_dz),
                loss=(loss, sum_bound(ls * e_lb.sum() + 2 * U * ls * lb.abs().sum(), ls * lb.abs().sum(), l0, loss,
                                      rpt + 6 + 4 + nb + 1)),
                correct=(correct, torch.full((1,), 0.25, dtype=torch.float64)))


LOSS_MUTANTS = ["mse_no_1_over_c", "ce_no_grad_scale", "loss_scale_ignored", "ties_take_last"]


def loss_emulate(p, kind, grad_scale, loss_scale, lbf16, mutant=None):
    z = p["z"].float()
    M, C = z.shape
    rl, dz = _loss32(z, p["y"].long(), kind, grad_scale, C, mutant)
    ls = 1.0 if mutant == "loss_scale_ignored" else loss_scale
    am = first_argmax(z)
    if mutant == "ties_take_last":
        am = C - 1 - first_argmax(z.flip(-1))
    return dict(dlogits=bf(dz) if lbf16 else dz, loss=p["loss0"] + rl.sum() * torch.tensor(ls, dtype=torch.float32),
                correct=p["correct0"] + (am == p["y"].long()).sum().float())
