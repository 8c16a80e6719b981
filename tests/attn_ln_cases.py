"""The per-op attention, LayerNorm and gather kernels as tables of cases, with fp64 references and derived error bounds.

csrc/attention.hip (attn_fwd_kernel, attn_bwd_kernel, attn_fwd_mfma<TT, DT>, attn_bwd_mfma<TT, DT>) and
csrc/nn_kernels.hip (layernorm_fwd_kernel, layernorm_fwd_small<LPR>, layernorm_bwd_kernel, layernorm_bwd_small<LPR>,
layernorm_bwd_fold, gather_rows16_kernel, gather_rows4_kernel): what a TabTransformer runs through ops/nn.py whenever
its shape is not the fused block's.  attn_kernel / ln_fwd_kernel / ln_bwd_kernel / gather_kernel name the kernel a case
reaches, computed from the launchers' own conditions.  The checking functions take the kernels' buffers in
tests/test_attn_ln_kernels_gpu.py and torch fp32 / bf16 emulations (with mutants) in tests/test_attn_ln_cases_cpu.py.

Bounds follow tests/tt_cases.py: u = 2^-24 per fp32 rounding, 2^-8 |value| per bf16 rounding, an accumulation of K terms
K u sum |terms| whatever the order, errors pushed through products and sums on magnitudes.  The same ASSUMPTION as
there, measured by nobody: the hardware transcendentals (and __expf, __logf, rsqrtf, 1.f / x and x / y built on them)
are granted one ulp, HW = 2 u relative; v_log_f32 near an argument of 1 is granted HW of 1; v_exp_f32 may flush a
subnormal result, FLUSH = 2^-126 absolute.

Attention.  These kernels work in the natural base: P = __expf(x), __expf(x) = v_exp_f32(x log2 e), so an exponent x
carries its own rounding, the constant's and the product's, 3 u |x|, then HW.  The row maximum m is whatever fp32 value
the kernel took: it shifts every exponent and is added back in lse = m + __logf(l), so it cancels exactly.
  scalar forward: q scale rounded to fp32, D accumulations ((D + 2) u scale |q|.|k| on a score, one u spare); the online
    softmax multiplies l and acc by alpha = __expf(m_old - m_new) at each of T steps: every step is charged alpha's HW
    and three roundings (the product by alpha, p v, the sum) of the whole sum of magnitudes; P stays fp32; 1.f / l is
    one HW and the product one u; o one bf16 rounding.
  MFMA forward: D accumulations, scores times scale (inside the same (D + 2) u), l a sum of T terms, P = e (1 / l)
    rounded to bf16 before P V (hidden), T accumulations, o rounded to bf16.
  backward: P = __expf(s scale - lse) on the forward's own lse (an exact input, so the backward's bound does not
    inherit the forward's error), delta = sum o do over D terms, dS = P (do.v - delta); scalar: dS and P stay fp32;
    MFMA: P rounded to bf16 in pass A (for dV) and dS rounded to bf16 in both passes (hidden); T accumulations; scale;
    each of dq, dk, dv one bf16 rounding.

LayerNorm.  Sums of N terms N u sum |terms| whatever the order (the generic kernel: 32 per-lane partials and a wave
reduction; the narrow kernels: 4 and log2(LPR) shuffles), divisions by N one HW.  The variance of the kernel is taken
about ITS mean m': sum (x - m')^2 = sum (x - m)^2 + N (m - m')^2 exactly, so the mean's error enters squared, not
through 2 |d| e_mean.  var' >= 0 whatever happened before, so var' + eps >= eps: where the variance's error bound
reaches var + eps (the VARIANCE CONDITION e_v < (var + eps) / 2 fails) rstd is still known to lie in
(0, eps^-1/2 (1 + HW)] and the bound says so instead of dividing by nothing.  The condition holds on every row of every
case except the one ill-conditioned row the edge set carries on purpose (magnitude 1e4, spread 1e-2: fp32 cannot hold
such a row's deviations, N u 1e4 is not small against 1e-2); tests/test_attn_ln_cases_cpu.py asserts exactly that.
dw / db: both backward launchers ADD into them; colsum_ref with the real number of adders (ln_bwd_adders).

A plain module, not a conftest: the tests import it."""
import functools
import itertools
import math

import numpy as np
import torch

from tt_cases import BF, FLUSH, HEAD_SCORE, HW, INPUT_SETS, bf, colsum_ref, mul_err, ratio, same_bits  # noqa: F401
from wide_step_cases import SECOND_ORDER, TINY, U

EPS = float(np.float32(1e-5))
F32, BF16 = torch.float32, torch.bfloat16


def f32scale(D):
    """1 / sqrt(D) as the fp32 value the launcher is handed: the references use this value, not the real one."""
    return float(np.float32(1.0 / math.sqrt(D)))


# ================================================================================================ attention
ATT_MAXD, ATT_MAXT, ATT_BWD_LDS = 64, 512, 160 * 1024


def A(T, D, Bsz=2, H=3, pad_q=0, pad_o=0, shift=None, fwd_only=False):
    """One attention call.  Rows are packed [q (H D) | k (H D) | v (H D) | pad_q] with ldq = 3 H D + pad_q and
    [o (H D) | pad_o] with ldo = H D + pad_o; ``shift``: elements by which a buffer starts off its 16-byte aligned
    allocation (qkv, o, do)."""
    return dict(T=T, D=D, Bsz=Bsz, H=H, pad_q=pad_q, pad_o=pad_o, shift=dict(shift or {}), fwd_only=fwd_only)


def att_name(c):
    s = "T%d_D%d_B%d_H%d" % (c["T"], c["D"], c["Bsz"], c["H"])
    s += "_padq%d_pado%d" % (c["pad_q"], c["pad_o"]) if c["pad_q"] or c["pad_o"] else ""
    s += "".join("_%s+%d" % kv for kv in sorted(c["shift"].items()))
    return s + ("_fwd" if c["fwd_only"] else "")


def att_ld(c):
    return 3 * c["H"] * c["D"] + c["pad_q"], c["H"] * c["D"] + c["pad_o"]


def attn_kernel(c, bwd):
    """The kernel dct_attention_fwd / dct_attention_bwd launches for the call, or "refused" (csrc/attention.hip:
    attn_mfma and the two launchers)."""
    T, D, HD = c["T"], c["D"], c["H"] * c["D"]
    if D > ATT_MAXD or T > ATT_MAXT or T < 1:
        return "refused"
    ldq, ldo = att_ld(c)
    sh = c["shift"]
    ptrs = [2 * (sh.get("qkv", 0) + i * HD) for i in range(3)]            # q, k, v: byte offsets off 16-byte alignment
    if bwd:
        ptrs += [2 * sh.get("o", 0), 2 * sh.get("do", 0)]
    if T % 16 == 0 and T <= 64 and D in (16, 32, 64) and ldq % 4 == 0 and ldo % 4 == 0 and not any(p % 8 for p in ptrs):
        return "attn_%s_mfma<%d, %d>" % ("bwd" if bwd else "fwd", T // 16, D // 16)
    if bwd and 8 * T * D + 4 + 8 * T > ATT_BWD_LDS:
        return "refused"
    return "attn_bwd_kernel" if bwd else "attn_fwd_kernel"


def is_mfma(name):
    return "mfma" in name


ATT_MFMA = [A(T, D, Bsz, H) for T in (16, 32, 48, 64) for D in (16, 32, 64) for Bsz, H in ((1, 1), (2, 3), (5, 1))]
ATT_MFMA.append(A(48, 32, pad_q=8, pad_o=4))
# every T with one D, every D with T = 17; 80 and 256 are MFMA-shaped but too long for it; 257 takes a second pass of
# the thread loops, 512 is the launcher's maximum
ATT_SCALAR = [A(1, 16), A(6, 5), A(15, 63), A(33, 40), A(80, 16), A(256, 64, Bsz=1, H=2), A(257, 1, Bsz=1, H=2)] \
    + [A(17, D) for D in (1, 5, 16, 40, 63, 64)] \
    + [A(512, 16, Bsz=1, H=2), A(512, 64, Bsz=1, H=2, fwd_only=True), A(17, 40, pad_q=3, pad_o=1)]
# MFMA-shaped calls that must take the scalar kernels (and meet their tighter bound): q / k / v 4 bytes off 8-byte
# alignment, a row stride that is no multiple of 4, and o alone off alignment (forward: MFMA, backward: scalar)
ATT_FALLBACK = [A(32, 32, shift={"qkv": 2}), A(32, 32, pad_q=2), A(32, 32, shift={"o": 2}), A(32, 32, shift={"do": 2})]
ATT_CASES = ATT_MFMA + ATT_SCALAR + ATT_FALLBACK
ATT_REFUSED = {"T = 0": A(0, 16), "T = 513": A(513, 16, Bsz=1, H=1), "D = 65": A(16, 65, Bsz=1, H=1)}
ATT_REFUSED_BWD_ONLY = {"backward at T = 512, D = 64": A(512, 64, Bsz=1, H=1)}


@functools.lru_cache(maxsize=None)
def _att_inputs(T, D, Bsz, H, kind):
    g = torch.Generator().manual_seed(7 + 1000 * T + 10 * D + 100003 * Bsz + 17 * H + (kind == "edge"))
    q, k, v, do = (torch.randn(Bsz, H, T, D, generator=g) for _ in range(4))
    for h in range(H):
        q[:, h] *= HEAD_SCORE[h % 4]
    if kind == "edge":  # scores out to several tens: a peaked softmax, P under FLUSH, large lse
        q, k = q * 3.0, k * 3.0
        do = do * 10.0 ** (-4.0 * torch.rand(Bsz, H, T, D, generator=g))
    return bf(q), bf(k), bf(v), bf(do)


def att_inputs(c, kind):
    """q, k, v, do as [Bsz][H][T][D] bf16 (read-only: shared between tests).  Every head's q has its own score scale;
    edge: q and k three times larger, do spanning 1e-4 .. 1."""
    return _att_inputs(c["T"], c["D"], c["Bsz"], c["H"], kind)


def rows(x):
    """[Bsz][H][T][D] -> the kernels' rows [Bsz * T][H * D]"""
    Bsz, H, T, D = x.shape
    return x.transpose(1, 2).reshape(Bsz * T, H * D)


def from_rows(x, Bsz, H):
    """[Bsz * T][H * D] -> [Bsz][H][T][D]"""
    M, HD = x.shape
    return x.reshape(Bsz, M // Bsz, H, HD // H).transpose(1, 2)


def attn_fwd_ref(q, k, v, scale, mfma):
    """(o, e_o, lse, e_lse), [Bsz][H][T][D] and [Bsz][H][T], of softmax(scale q k^T) v on the bf16 inputs; the
    roundings counted in the module docstring."""
    q, k, v = q.double(), k.double(), v.double()
    T, D = q.shape[-2:]
    kt = k.transpose(-1, -2)
    y, sabs = (q @ kt) * scale, q.abs() @ kt.abs()
    ymax = y.max(-1, keepdim=True).values
    e_y = (D + 2) * U * scale * sabs + 3 * U * (ymax - y)
    lse = torch.logsumexp(y, -1, keepdim=True)
    P = torch.exp(y - lse)
    rel = torch.expm1(e_y) + HW
    step = T * U if mfma else T * (HW + 3 * U)
    rl = (P * rel).sum(-1, keepdim=True) * SECOND_ORDER + step
    assert bool((rl < 0.5).all())
    eP = ((1 + rel) * (1 + HW + U) / (1 - rl) - 1) * P + T * FLUSH
    if mfma:
        eP = eP + BF * (P + eP)
    o = P @ v
    e_o = eP @ v.abs() + step * ((P + eP) @ v.abs())
    e_o = BF * (o.abs() + e_o) + e_o + TINY
    logl = lse - ymax
    e_lse = -torch.log1p(-rl) + HW * (logl + 1.0) + U * logl + U * lse.abs() + TINY
    return o, e_o, lse[..., 0], e_lse[..., 0]


def attn_bwd_ref(q, k, v, o, lse, do, scale, mfma):
    """{dq, dk, dv: (value, bound)} of the flash-form backward as the kernels define it, on the given bf16 q, k, v, o,
    do and fp32 lse: P = exp(scale q.k - lse) (no renormalisation), delta = sum do o, dS = P (do.v - delta),
    dv = P^T do, dk = scale dS^T q, dq = scale dS k."""
    q, k, v, o, do = (x.double() for x in (q, k, v, o, do))
    T, D = q.shape[-2:]
    kt, vt = k.transpose(-1, -2), v.transpose(-1, -2)
    lq = lse.double()[..., None]
    y, sabs = (q @ kt) * scale, q.abs() @ kt.abs()
    x = y - lq
    e_x = (D + 2) * U * scale * sabs + 3 * U * x.abs()
    P = torch.exp(x)
    eP = (torch.expm1(e_x) + HW) * P + FLUSH
    delta = (do * o).sum(-1, keepdim=True)
    e_delta = D * U * (do.abs() * o.abs()).sum(-1, keepdim=True)
    dP = do @ vt
    e_dP = D * U * (do.abs() @ vt.abs())
    w = dP - delta
    e_w = e_dP + e_delta + U * w.abs()
    dS = P * w
    e_dS = mul_err(P, eP, w, e_w) + U * dS.abs()
    if mfma:  # the hidden roundings: P (pass A), dS (both passes)
        eP = eP + BF * (P + eP)
        e_dS = e_dS + BF * (dS.abs() + e_dS)
    Pt, ePt, dSt, e_dSt = (z.transpose(-1, -2) for z in (P, eP, dS, e_dS))
    dv = Pt @ do
    e_dv = ePt @ do.abs() + T * U * ((Pt + ePt) @ do.abs())
    dk = scale * (dSt @ q)
    e_dk = scale * (e_dSt @ q.abs() + T * U * ((dSt.abs() + e_dSt) @ q.abs())) + U * dk.abs()
    dq = scale * (dS @ k)
    e_dq = scale * (e_dS @ k.abs() + T * U * ((dS.abs() + e_dS) @ k.abs())) + U * dq.abs()
    fin = lambda z, e: BF * (z.abs() + e) + e * SECOND_ORDER + TINY  # noqa: E731
    return {"dq": (dq, fin(dq, e_dq)), "dk": (dk, fin(dk, e_dk)), "dv": (dv, fin(dv, e_dv))}


def attn_fwd_check(got, q, k, v, scale, mfma):
    o, e_o, lse, e_lse = attn_fwd_ref(q, k, v, scale, mfma)
    return {"o": ratio(got["o"], o, e_o), "lse": ratio(got["lse"], lse, e_lse)}


def attn_bwd_check(got, q, k, v, o, lse, do, scale, mfma):
    ref = attn_bwd_ref(q, k, v, o, lse, do, scale, mfma)
    return {n: ratio(got[n], *ref[n]) for n in ("dq", "dk", "dv")}


def _heaviest_key(s):
    """Batch 0, head 0: the key with the largest softmax weight summed over the queries."""
    return int(torch.softmax(s[0, 0].double(), -1).sum(0).argmax())


def emulate_attn_fwd(q, k, v, scale, mfma, mutant=None):
    """The forward in torch fp32 with the kernels' rounding sites: scalar - q scale, the online softmax key by key;
    MFMA - scores times scale, one maximum, P = bf16(e (1 / l)).  ``mutant``: one of ATT_FWD_MUTANTS."""
    sc = torch.tensor(scale, dtype=F32)
    q, k, v = q.float(), k.float(), v.float()
    T = q.shape[-2]
    kt = k.transpose(-1, -2)
    if mfma:
        s = (q @ kt) * sc
        if mutant == "key_dropped":
            s[0, 0, :, _heaviest_key(s)] = -math.inf
        m = s.max(-1, keepdim=True).values
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        pr = e * (1.0 / l)
        if mutant == "p_not_divided":
            i = int(l[0, 0, :, 0].argmax())
            pr[0, 0, i] = e[0, 0, i]
        o = bf(pr).float() @ v
    else:
        s = (q * sc) @ kt
        if mutant == "key_dropped":
            s[0, 0, :, _heaviest_key(s)] = -math.inf
        m = torch.full(s.shape[:-1], -3.402823466e+38)
        l, acc = torch.zeros_like(m), torch.zeros_like(q)
        for j in range(T):
            mn = torch.maximum(m, s[..., j])
            alpha, p = torch.exp(m - mn), torch.exp(s[..., j] - mn)
            l = l * alpha + p
            acc = acc * alpha[..., None] + p[..., None] * v[..., j:j + 1, :]
            m = mn
        inv = 1.0 / l
        if mutant == "p_not_divided":
            inv[0, 0, int(l[0, 0].argmax())] = 1.0
        o, m, l = acc * inv[..., None], m[..., None], l[..., None]
    o = bf(o)
    if mutant == "heads_swapped" and o.shape[1] > 1:
        o = o[:, [1, 0] + list(range(2, o.shape[1]))]
    lse = m if mutant == "lse_without_log_l" else m + torch.log(l)
    return {"o": o, "lse": lse[..., 0]}


def emulate_attn_bwd(q, k, v, o, lse, do, scale, mfma, mutant=None):
    """The backward in torch fp32; MFMA: bf16 P for dV and bf16 dS.  ``mutant``: one of ATT_BWD_MUTANTS."""
    sc = torch.tensor(scale, dtype=F32)
    q, k, v, o, do = (x.float() for x in (q, k, v, o, do))
    T = q.shape[-2]
    P = torch.exp((q @ k.transpose(-1, -2)) * sc - lse[..., None])
    delta = (do * o).sum(-1, keepdim=True)
    if mutant == "delta_omitted":
        delta = torch.zeros_like(delta)
    dS = P * (do @ v.transpose(-1, -2) - delta)
    Pv = P
    if mfma:
        dS, Pv = bf(dS).float(), bf(P).float()
    if mutant == "dv_wrong_query_tile" and T >= 32:  # P's query tiles 0 and 1 swapped under dV = P^T dO
        Pv = torch.cat([Pv[..., 16:32, :], Pv[..., :16, :], Pv[..., 32:, :]], -2)
    dv = Pv.transpose(-1, -2) @ do
    dk = dS.transpose(-1, -2) @ q
    if mutant != "dk_without_scale":
        dk = dk * sc
    dq = (dS @ k) * sc
    return {"dq": bf(dq), "dk": bf(dk), "dv": bf(dv)}


# mutant -> the tensor whose ratio must exceed 1 on at least one case
ATT_FWD_MUTANTS = {"key_dropped": "o", "heads_swapped": "o", "p_not_divided": "o", "lse_without_log_l": "lse"}
ATT_BWD_MUTANTS = {"dk_without_scale": "dk", "delta_omitted": "dq", "dv_wrong_query_tile": "dv"}


# ================================================================================================ LayerNorm
LN_MAXN, LN_NSLOT = 2048, 16
CONST_ROW, CONST_VAL, BIG_ROW, BIG_VAL, BIG_SPREAD = 0, 0.3, 1, 1.0e4, 1.0e-2

LN_FWD_NS = (1, 3, 4, 8, 12, 20, 48, 64, 68, 132, 192, 252, 256, 260, 1000, 2048)
LN_MS = (1, 5, 37)
LN_FWD_DTYPES = ((0, 0), (0, 1), (1, 0), (1, 1))          # (in_bf16, out_bf16)
LN_FWD_BIG = (16400, 256)                                 # a second grid-stride pass of layernorm_fwd_small<64>
LN_FWD_NULLS = ("w", "b", "wb", "stats")                  # operands passed as null, at (37, 64) and (37, 260)
LN_BWD_EX_NS = (4, 8, 12, 20, 48, 64, 68, 132, 252, 256)
LN_BWD_EX_BIG = ((300, 64), (4200, 256))                  # 19 blocks: slot rows shared; 1050 > 1024 blocks: two passes
# (dy_bf16, x_bf16, dx_bf16, dx2, dres): the three ops/nn.py uses first, then every other combination
LN_BWD_EX_USED = ((1, 0, 0, 1, 1), (1, 0, 0, 0, 0), (1, 0, 1, 0, 0))
LN_BWD_EX_MODES = LN_BWD_EX_USED + tuple(m for m in itertools.product((0, 1), repeat=5) if m not in LN_BWD_EX_USED)
LN_BWD_EX_GRADS = ("wb", "w", "b", "")                    # which of dw / db are passed
LN_BWD_NS = (1, 3, 64, 260, 1000, 2048)
LN_BWD_BIG = ((4200, 3), (4200, 260))                     # 1050 > 1024 blocks: a second grid-stride pass
LN_BWD_EX_REFUSED = {"N % 4": dict(N=6), "N > 256": dict(N=260), "null workspace": dict(N=64, ws=False),
                     "misaligned dres": dict(N=64, shift="dres"), "misaligned dx2": dict(N=64, shift="dx2"),
                     "misaligned w": dict(N=64, shift="w"), "misaligned w, N = 1000": dict(N=1000, shift="w")}


def ln_lpr(N, aligned=True):
    """Lanes per row of the narrow kernels; 0: they cannot take the call (csrc/nn_kernels.hip ln_lpr)."""
    if N % 4 or N > 256 or not aligned:
        return 0
    lpr = 1
    while lpr * 4 < N:
        lpr *= 2
    return lpr


def ln_fwd_kernel(M, N, aligned=True):
    """``aligned``: x, y, w and b all on 16-byte boundaries (null counts as aligned)."""
    if N > LN_MAXN:
        return "refused"
    lpr = ln_lpr(N, aligned)
    return "layernorm_fwd_small<%d>" % lpr if lpr else "layernorm_fwd_kernel"


def ln_fwd_passes(M, N, aligned=True):
    """Grid-stride passes of the forward: the narrow grid caps at 4096 blocks of 4 (64 / LPR) rows."""
    lpr = ln_lpr(N, aligned)
    if not lpr:
        return 1
    rpb = 4 * (64 // lpr)
    return -(-M // (rpb * min(4096, -(-M // rpb))))


def ln_bwd_kernel(M, N, ex, aligned=True, ws=True):
    if ex:
        lpr = ln_lpr(N, aligned)
        return "layernorm_bwd_small<%d>" % lpr if lpr and ws else "refused"
    return "refused" if N > LN_MAXN else "layernorm_bwd_kernel"


def ln_bwd_fold_runs(grads):
    """layernorm_bwd_fold follows the row kernel whenever dw or db is passed."""
    return bool(grads)


def ln_bwd_grid(M, N, ex):
    rpb = 4 * (64 // ln_lpr(N)) if ex else 4
    return rpb, max(1, min(1024, -(-M // rpb)))


def ln_bwd_row_block(M, N):
    """The block of layernorm_bwd_small that owns each row (row r: lane group r mod RPW of wave (r / RPW) mod waves)."""
    lpr = ln_lpr(N)
    rpb, grid = ln_bwd_grid(M, N, True)
    return ((torch.arange(M) // (64 // lpr)) % (grid * 4)) // 4


def ln_bwd_adders(M, N, ex):
    """fp32 additions on the longest path from a row's term into dw / db.  Narrow: a lane group's rows over the
    grid-stride passes, the block's 256 / LPR partials, the blocks sharing a slot row (atomics), the 16 slot rows, the
    += into dw.  Generic: a wave's rows over the passes, the 4 waves, one atomic per block into dw itself."""
    rpb, grid = ln_bwd_grid(M, N, ex)
    passes = -(-M // (rpb * grid))
    if ex:
        return passes + 256 // ln_lpr(N) + -(-grid // LN_NSLOT) + LN_NSLOT + 1
    return passes + 4 + grid


@functools.lru_cache(maxsize=8)
def ln_inputs(M, N, kind, in_bf16=0, dy_bf16=0):
    """x, w, b, dy, dres, dw0, db0 (read-only: shared).  edge: row 0 constant; row 1 of magnitude 1e4 with spread 1e-2;
    dy spanning 1e-4 .. 1.  bf16 operands hold bf16 values."""
    g = torch.Generator().manual_seed(31 + 1000 * M + N + (kind == "edge"))
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x, dy = r(M, N) * 1.5 + 0.25, r(M, N)
    if kind == "edge":
        x[CONST_ROW] = CONST_VAL
        if M > BIG_ROW:
            x[BIG_ROW] = BIG_VAL + BIG_SPREAD * r(N)
        dy = dy * 10.0 ** (-4.0 * torch.rand(M, N, generator=g))
    if in_bf16:
        x = bf(x)
    if dy_bf16:
        dy = bf(dy)
    return dict(x=x, w=1 + 0.1 * r(N), b=0.1 * r(N), dy=dy, dres=r(M, N), dw0=r(N), db0=r(N))


def ln_ref(x, w, b, out_bf16):
    """LayerNorm over the N columns of exactly known rows x [M][N] (fp64): mean, rstd, y with bounds, and ``cond``,
    the variance condition row by row (module docstring)."""
    M, N = x.shape
    w = torch.ones(N, dtype=torch.float64) if w is None else w.double()
    b = torch.zeros(N, dtype=torch.float64) if b is None else b.double()
    mean = x.mean(-1, keepdim=True)
    e_mean = N * U * x.abs().mean(-1, keepdim=True) + HW * mean.abs()
    d = x - mean
    e_d = e_mean + U * (d.abs() + e_mean)
    var = (d * d).mean(-1, keepdim=True)
    varp = var + e_mean * e_mean          # the kernel's variance about its own mean, at most
    # d's rounding twice, the square's once, one spare; the sum; the division
    e_var = e_mean * e_mean + (4 * U + N * U + HW) * varp * SECOND_ORDER
    v = var + EPS
    e_v = e_var + U * (v + e_var)
    cond = (e_v < 0.5 * v)[:, 0]
    v_lo = torch.maximum(v - e_v, torch.full_like(v, EPS))
    rstd = v ** -0.5
    e_rstd = torch.maximum(v_lo ** -0.5 * (1 + HW) - rstd, rstd - (v + e_v) ** -0.5 * (1 - HW)) * SECOND_ORDER
    xh = d * rstd
    e_xh = mul_err(d, e_d, rstd, e_rstd) + U * (xh.abs() + mul_err(d, e_d, rstd, e_rstd))
    y = xh * w + b
    e_y = (e_xh * w.abs() + U * (xh.abs() + e_xh) * w.abs()) * SECOND_ORDER
    e_y = e_y + U * (y.abs() + e_y)
    if out_bf16:
        e_y = BF * (y.abs() + e_y) + e_y
    return dict(mean=mean[:, 0], e_mean=e_mean[:, 0] + TINY, rstd=rstd[:, 0], e_rstd=e_rstd[:, 0] + TINY, y=y,
                e_y=e_y + TINY, cond=cond)


def ln_fwd_check(got, x, w, b, out_bf16):
    r = ln_ref(x.double(), w, b, out_bf16)
    out = {"y": ratio(got["y"], r["y"], r["e_y"])}
    if got.get("mean") is not None:
        out["mean"] = ratio(got["mean"], r["mean"], r["e_mean"])
        out["rstd"] = ratio(got["rstd"], r["rstd"], r["e_rstd"])
    return out


def emulate_ln_fwd(x, w, b, out_bf16, mutant=None):
    """The forward kernels op by op in torch fp32.  ``mutant``: one of LN_FWD_MUTANTS."""
    M, N = x.shape
    x, n = x.float(), torch.tensor(float(N), dtype=F32)
    mean = x.sum(-1, keepdim=True) / n
    if mutant == "mean_over_n_minus_1":  # the last row's mean without its last column
        mean[M - 1] = x[M - 1, :max(N - 1, 1)].sum() / n
    d = x if mutant == "variance_about_zero" else x - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / n + (0.0 if mutant == "eps_omitted" else EPS))
    y = (x - mean) * rstd * (1.0 if w is None else w) + (0.0 if b is None else b)
    return {"y": bf(y) if out_bf16 else y, "mean": mean[:, 0].contiguous(), "rstd": rstd[:, 0].contiguous()}


# "variance_about_zero" is asked of rstd; "eps_omitted" shows on the constant row (rstd = inf or 1e8)
LN_FWD_MUTANTS = {"mean_over_n_minus_1": "mean", "variance_about_zero": "rstd", "eps_omitted": "rstd"}


def ln_bwd_ref(dy, x, w, mean, rstd, dres, dw0, db0, adders, dx_bf16):
    """dx, dw, db with bounds, from the SAVED fp32 mean / rstd (exact inputs of the backward):
    dx = rstd (g - mean g - xh mean(g xh)) [+ dres], g = dy w, xh = (x - mean) rstd; dw = dw0 + sum dy xh,
    db = db0 + sum dy."""
    dy, x = dy.double(), x.double()
    M, N = x.shape
    w = torch.ones(N, dtype=torch.float64) if w is None else w.double()
    rs = rstd.double()[:, None]
    d = x - mean.double()[:, None]
    xh = d * rs
    e_xh = U * d.abs() * rs + U * xh.abs()
    gw = dy * w
    e_gw = U * gw.abs()
    s1 = gw.mean(-1, keepdim=True)
    e_s1 = e_gw.mean(-1, keepdim=True) + N * U * gw.abs().mean(-1, keepdim=True) + HW * s1.abs()
    gx = gw * xh
    e_gx = mul_err(gw, e_gw, xh, e_xh) + U * gx.abs()
    s2 = gx.mean(-1, keepdim=True)
    e_s2 = e_gx.mean(-1, keepdim=True) + N * U * gx.abs().mean(-1, keepdim=True) + HW * s2.abs()
    xs = xh * s2
    e_xs = mul_err(xh, e_xh, s2, e_s2) + U * xs.abs()
    t = gw - s1 - xs
    e_t = e_gw + e_s1 + e_xs + U * (gw - s1).abs() + U * t.abs()
    r = rs * t
    e_r = rs * e_t + U * r.abs()
    dx, e_dx = r, e_r
    if dres is not None:
        dx = r + dres.double()
        e_dx = e_r + U * dx.abs()
    e_dx = e_dx * SECOND_ORDER + TINY
    if dx_bf16:
        e_dx = BF * (dx.abs() + e_dx) + e_dx
    tw = dy * xh
    e_tw = dy.abs() * e_xh + U * tw.abs()
    return {"dx": (dx, e_dx), "dw": colsum_ref(tw, e_tw, dw0, adders),
            "db": colsum_ref(dy, torch.zeros_like(dy), db0, adders)}


def ln_bwd_check(got, dy, x, w, mean, rstd, dres, dw0, db0, adders, dx_bf16):
    ref = ln_bwd_ref(dy, x, w, mean, rstd, dres, dw0, db0, adders, dx_bf16)
    return {k: ratio(got[k], *ref[k]) for k in ("dx", "dw", "db") if got.get(k) is not None}


def emulate_ln_bwd(dy, x, w, mean, rstd, dres, dw0, db0, dx_bf16, mutant=None, row_block=None):
    """The backward kernels op by op in torch fp32.  ``mutant``: one of LN_BWD_MUTANTS; ``row_block``
    (ln_bwd_row_block) places the rows into slot rows for "slot_row_left_out"."""
    dy, x = dy.float(), x.float()
    M, N = x.shape
    n = torch.tensor(float(N), dtype=F32)
    w1 = torch.ones(N) if w is None else w
    xh = (x - mean[:, None]) * rstd[:, None]
    gw = dy * w1
    s1 = gw.sum(-1, keepdim=True) / n
    s2 = (gw * xh).sum(-1, keepdim=True) / n
    if mutant == "mean_g_xhat_dropped":
        s2 = torch.zeros_like(s2)
    dx = rstd[:, None] * (gw - s1 - xh * s2)
    if dres is not None and mutant != "dres_not_added":
        dx = dx + dres
    tw, tb = (gw if mutant == "dw_from_g_w" else dy) * xh, dy
    if mutant == "slot_row_left_out":  # the fold stops one slot row short
        keep = (row_block % LN_NSLOT != min(LN_NSLOT, int(row_block.max()) + 1) - 1).float()[:, None]
        tw, tb = tw * keep, tb * keep
    return {"dx": bf(dx) if dx_bf16 else dx, "dw": dw0 + tw.sum(0), "db": db0 + tb.sum(0)}


LN_BWD_MUTANTS = {"mean_g_xhat_dropped": "dx", "dres_not_added": "dx", "dw_from_g_w": "dw", "slot_row_left_out": "db"}


# ================================================================================================ gather
# name -> (n_rows, row_bytes, source rows, byte shift of the source, index list)
GATHER_GRID_VECTORS = 2048 * 256


def G(n_rows, row_bytes, src_rows, shift=0, idx="random"):
    return dict(n_rows=n_rows, row_bytes=row_bytes, src_rows=src_rows, shift=shift, idx=idx)


GATHER_CASES = {
    "48-byte rows": G(37, 48, 11),
    "1024-byte rows": G(37, 1024, 50),
    "20-byte rows": G(37, 20, 11),
    "48-byte rows, source 4 bytes off": G(37, 48, 11, shift=4),
    "repeated indices": G(40, 48, 11, idx="repeated"),
    "first and last index": G(2, 48, 11, idx="ends"),
    "one row": G(1, 1024, 5),
    "one row of words": G(1, 20, 5),
    "second grid-stride pass": G(8200, 1024, 300),
    "second grid-stride pass of words": G(26300, 80, 300, shift=4),
}
GATHER_REFUSED = {"row_bytes = 6": G(5, 6, 11)}
GATHER_EMPTY = {"n_rows = 0": G(0, 48, 11)}


def gather_kernel(c):
    """csrc/nn_kernels.hip dct_gather_rows (the destination is 16-byte aligned in every case)."""
    if c["n_rows"] <= 0:
        return "nothing"
    if c["row_bytes"] % 16 == 0 and c["shift"] % 16 == 0:
        return "gather_rows16_kernel"
    return "gather_rows4_kernel" if c["row_bytes"] % 4 == 0 else "refused"


def gather_passes(c):
    unit = 16 if gather_kernel(c) == "gather_rows16_kernel" else 4
    return -(-(c["n_rows"] * (c["row_bytes"] // unit)) // GATHER_GRID_VECTORS)


def gather_inputs(c, seed=41):
    """(src bytes [src_rows][row_bytes] uint8, idx int32 [n_rows])"""
    g = torch.Generator().manual_seed(seed + c["n_rows"] + c["row_bytes"])
    src = torch.randint(0, 256, (c["src_rows"], c["row_bytes"]), generator=g, dtype=torch.int32).to(torch.uint8)
    n, last = c["n_rows"], c["src_rows"] - 1
    if c["idx"] == "repeated":
        idx = torch.randint(0, 3, (n,), generator=g)
    elif c["idx"] == "ends":
        idx = torch.tensor([last, 0])
    else:
        idx = torch.randint(0, last + 1, (n,), generator=g)
        if n >= 2:
            idx[0], idx[n - 1] = last, 0
    return src, idx.to(torch.int32)


def gather_ref(src, idx):
    return src[idx.long()]
