"""The wide-MLP step's launchers as tables of cases, with their fp64 references and derived error bounds.

Flat Adam (csrc/adam_impl.h, optim.hip), the split-K dW partials with Adam riding along and the gathered first forward
GEMM (csrc/gemm_bf16.hip), and the step bookkeeping kernels (csrc/step_kernels.hip).  Every reference is torch float64
on the CPU; every bound is counted from the fp32 operations of the kernel it bounds, with u = 2^-24 the unit roundoff
of one fp32 operation.  tests/test_wide_step_cases_cpu.py runs the references against their own bounds and the tables
against the launchers' preconditions; tests/test_wide_step_kernels_gpu.py launches them.

A plain module, not a conftest: the tests import it."""
import math
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24           # unit roundoff of one fp32 operation (round to nearest)
TINY = 2.0 ** -149       # the smallest fp32 subnormal: the absolute error of a rounding that underflows
SECOND_ORDER = 1.0 + 2.0 ** -18  # products of the <= 32 roundings counted below, (1 + u)^32 - 1 - 32 u < 2^-18 * 32 u


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ flat Adam
Hyper = namedtuple("Hyper", "lr b1 b2 eps wd grad_scale decoupled")
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
DECAYS = [(0.0, 0), (0.05, 0), (0.05, 1)]  # (wd, decoupled)
GRAD_SCALES = [1.0, 0.125]
STEPS = [1, 2, 10, 1000]
HYPERS = [Hyper(LR, B1, B2, EPS, wd, gs, dec) for wd, dec in DECAYS for gs in GRAD_SCALES]

# n -> what it is the edge of.  One launch is <= 2048 workgroups of 256 threads, a float4 each.
ADAM_NS = {
    4099: "n % 4 == 3: the scalar tail of the range that ends the buffer",
    4096: "whole float4s, no tail",
    3: "tail only: no float4 at all",
    1037: "tail 1, a partly filled last workgroup",
    600000: "586 workgroups, every one full (one pass: a launch holds 2048 * 256 float4s)",
}
ADAM_N_TWO_PASSES = 4 * 2048 * 256 + 4 * 300 + 3  # 2048 workgroups, a second grid-stride pass of 300 float4s, tail 3
# launcher -> the kernel it reaches (csrc/optim.hip)
ADAM_LAUNCHERS = {
    "adam_flat": "adam_flat_kernel<false>",
    "adam_flat_step": "adam_flat_kernel<false>",
    "adam_flat_step_parts": "adam_flat_kernel<true, 4>",
    "adam_range": "adam_range_kernel<4>",
}

# split-K partials standing in for g: (name, n, [(offset, count, splits)], kernel).  Ranges are not adjacent (the gaps
# read g); with n % 4 == 3 one range ends at n & ~3, so the tail reads g.
PART_SLOTS = 8  # slice slots allocated per range: those past `splits` hold NaN
PARTS_CASES = [
    ("s148", 4099, [(8, 1024, 1), (1200, 2048, 4), (3584, 512, 8)], "adam_flat_kernel<true, 8>"),
    ("s234", 4099, [(8, 1024, 2), (1200, 2048, 3), (3584, 512, 4)], "adam_flat_kernel<true, 4>"),
    ("s5", 4099, [(1024, 2048, 5)], "adam_flat_kernel<true, 8>"),
]
RANGE_N = 4099
RANGES = [(0, 2048), (2048, RANGE_N), (1024, 1028)]  # [lo, hi) of dct_adam_range; the second carries the tail


def adam_inputs(n, scale, seed):
    """p, g, m, v fp32 on the CPU.  "tabular": the magnitudes of the tabular step (g ~ 1e-4, m ~ 1e-5, v 1e-12 ..
    1e-8, log-uniform); "unit": everything O(1)."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(n, generator=gen)  # noqa: E731
    if scale == "tabular":
        p, g, m = r() * 0.05, r() * 1e-4, r() * 1e-5
        v = 10.0 ** (torch.rand(n, generator=gen) * 4 - 12)
    else:
        p, g, m = r(), r(), r()
        v = torch.rand(n, generator=gen) + 1e-3
    return p.float(), g.float(), m.float(), v.float()


def part_slices(ranges, scale, seed):
    """One [PART_SLOTS][count] fp32 buffer per range: slices [0, splits) random at g's magnitude / splits, the
    unused slots NaN."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for off, cnt, sp in ranges:
        s = torch.full((PART_SLOTS, cnt), float("nan"))
        s[:sp] = torch.randn(sp, cnt, generator=gen) * ((1e-4 if scale == "tabular" else 1.0) / sp)
        out.append(s.float())
    return out


def bias_corrections(hp, t, device_counter):
    """(step_size, rbc2, c1, c2): lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) as the path computes them, and the relative
    error c1 / c2 the bound grants each.

    Host t (optim.hip dct_adam_flat_step): both in double from the fp32 hyper-parameters, then cast to float - the
    reference makes the same cast, so the cast costs the bound nothing.
    Device counter (adam_impl.h adam_bias_correction): 1 - exp2(t * log2f(b)) in fp32.  b^t rounded to fp32 is off by
    up to 2^-24 absolute and the subtraction cancels down to 1 - b^t, so each correction is granted the relative
    error 2^-23 / (1 - b^t) against the exact fp64 value (plus u for step_size's fp32 division)."""
    lr, b1, b2 = f32(hp.lr), f32(hp.b1), f32(hp.b2)
    bc1, bc2 = 1.0 - math.pow(b1, t), 1.0 - math.pow(b2, t)
    if not device_counter:
        return f32(lr / bc1), f32(1.0 / math.sqrt(bc2)), 0.0, 0.0
    return lr / bc1, 1.0 / math.sqrt(bc2), 2.0 ** -23 / bc1 + U, 2.0 ** -23 / bc2


AdamRef = namedtuple("AdamRef", "p m v p_bound m_bound v_bound upd")


def adam_ref(p, g, m, v, t, hp, parts=None, lo=0, hi=None, device_counter=False):
    """adam_one (csrc/adam_impl.h) in fp64 over elements [lo, hi) of fp32 inputs; elements outside are returned
    unchanged.  ``parts``: [(offset, count, splits, slices [>= splits][count])] - g over such a range is the fp64 sum
    of its first ``splits`` slices.  Hyper-parameters are rounded to fp32 first, and 1 - b as the fp32 difference.

    Returns the new p, m, v (fp64), the absolute error bounds of an fp32 evaluation, and Adam's update step_size m' / D
    alone (without decoupled decay's share of p_old - p_new).

    Bounds, u = 2^-24 per fp32 rounding, each rounding relative to an intermediate that the sum of the absolute values
    of the terms bounds:
      g_eff = grad_scale * g (+ wd * p): sp - 1 additions of the slice sum, 1 scaling, and coupled decay's product
              and addition: Ng = sp + 2 roundings of G = grad_scale * sum|slice| + wd |p|.
      m' = b1 m + (1 - b1) g_eff: 3 roundings of its own plus g_eff's Ng -> (Ng + 3) u Tm, Tm = b1 |m| + (1 - b1) G.
      v' = b2 v + (1 - b2) g_eff^2: 4 roundings of its own; g_eff enters squared, so its Ng count twice
           -> (2 Ng + 4) u Tv, Tv = b2 v + (1 - b2) G^2.
      p' = p (- lr wd p) - step_size m' / (sqrt(v') rbc2 + eps).  hipcc's default keeps sqrtf and the division
           correctly rounded (no fast-math flag in _build.py), so the update U costs
             step_size bm / D            (m's bound through the quotient)
           + |U| (2 u + eD / (D - eD))   (product, division; the denominator's error)
           with D = sqrt(v') rbc2 + eps and eD = rbc2 (sqrt(v') - sqrt(v' - bv)) + 3 u D (v's bound through the
           concave sqrt, then sqrt, product, sum), plus |U| (c1 + c2) on the device-counter path
           (bias_corrections).  That much is in units of the update.  In units of p: u (|p| + |U|) for the final
           subtraction, and for decoupled decay the same again plus 2 u lr wd |p| - together at most one ulp of p."""
    n = p.numel()
    hi = n if hi is None else hi
    lr, b1, b2, eps, wd, gs = (f32(x) for x in (hp.lr, hp.b1, hp.b2, hp.eps, hp.wd, hp.grad_scale))
    omb1, omb2 = f32(np.float32(1) - np.float32(b1)), f32(np.float32(1) - np.float32(b2))
    p0, m0, v0 = p.double(), m.double(), v.double()
    g_eff, g_abs = g.double().clone(), g.double().abs()
    ng = torch.full((n,), 1.0 + 2.0, dtype=torch.float64)
    for off, cnt, sp, slices in parts or []:
        s = slices[:sp].double()
        g_eff[off:off + cnt] = s.sum(0)
        g_abs[off:off + cnt] = s.abs().sum(0)
        ng[off:off + cnt] = sp + 2.0
    step_size, rbc2, c1, c2 = bias_corrections(hp, t, device_counter)
    g_eff, G = g_eff * gs, g_abs * gs
    pd = p0
    p_abs = U * p0.abs()  # the final subtraction
    if hp.decoupled:
        pd = p0 - lr * wd * p0
        p_abs = p_abs + U * p0.abs() + 2 * U * lr * wd * p0.abs()
    else:
        g_eff, G = g_eff + wd * p0, G + wd * p0.abs()
    m1 = b1 * m0 + omb1 * g_eff
    v1 = b2 * v0 + omb2 * g_eff * g_eff
    bm = (ng + 3) * U * (b1 * m0.abs() + omb1 * G) * SECOND_ORDER + 6 * TINY
    bv = (2 * ng + 4) * U * (b2 * v0 + omb2 * G * G) * SECOND_ORDER + 8 * TINY
    sq = v1.sqrt()
    D = sq * rbc2 + eps
    eD = rbc2 * (sq - (v1 - bv).clamp_min(0).sqrt()) + 3 * U * D
    upd = step_size * m1 / D
    bu = step_size * bm / D + upd.abs() * (2 * U + eD / (D - eD) + c1 + c2) * SECOND_ORDER
    p1 = pd - upd
    bp = bu + p_abs + U * upd.abs() + 2 * TINY
    inside = torch.zeros(n, dtype=torch.bool)
    inside[lo:hi] = True
    zero = torch.zeros(n, dtype=torch.float64)
    return AdamRef(torch.where(inside, p1, p0), torch.where(inside, m1, m0), torch.where(inside, v1, v0),
                   torch.where(inside, bp, zero), torch.where(inside, bm, zero), torch.where(inside, bv, zero),
                   torch.where(inside, upd, zero))


# ------------------------------------------------------------------------------------------------ gather
def gather_rows_ref(idx, cursor, stride, n_items, M):
    """Dataset rows of a batch (csrc/kernels.h GatherFwd / dct_gather_batch): row m is idx[q], q = cursor * stride + m,
    q % n_items when q >= n_items."""
    q = cursor * stride + torch.arange(M, dtype=torch.int64)
    q = torch.where(q < n_items, q, q % n_items)
    return idx.long()[q]


# (offset, count) of the ranges the prologues clear in a NaN-filled buffer of ZERO_LEN floats: a 3-element tail, whole
# float4s, a long range with a 2-element tail, an empty one.  Element 7 and everything from 2054 on stay NaN.
ZERO_RANGES = [(0, 7), (8, 4), (1024, 1030), (4096, 0)]
ZERO_LEN = 4104


def zero_mask():
    z = torch.zeros(ZERO_LEN, dtype=torch.bool)
    for off, cnt in ZERO_RANGES:
        z[off:off + cnt] = True
    return z


# ------------------------------------------------------------------------------------------------ GEMMs
GBK = 64  # k per LDS stage of the LDS-DMA kernels (csrc/gemm_bf16.hip)


def gemm_ref(a, b):
    """(a b, |a| |b|) in fp64 for bf16 operands a [M][K], b [K][N] widened to fp64 (a bf16 product is exact in fp32
    and in fp64)."""
    a, b = a.double(), b.double()
    return a @ b, a.abs() @ b.abs()


def partial_bound(ref, absprod, k_slice):
    """fp32-out split-K partial: k_slice fp32 accumulations, each rounding an intermediate that sum|a||b| bounds
    (whatever order the MFMA adds in), plus one rounding of the result."""
    return (k_slice * U * absprod + U * ref.abs()) * SECOND_ORDER + TINY


def fwd_bound(z, absprod, K):
    """bf16-out forward z = a w^T + bias: the fp32 accumulation bound, plus 2^-8 |z| for the rounding to bf16 (8
    significant bits: unit roundoff 2^-8 / (1 + 2^-8)).  The fp32 bias add's u |z| and the rounding's share of the
    accumulation error (2^-8 of it) sit in the slack of K u sum|a||b|, which charges every one of the K products a
    rounding of the whole sum.  ReLU is 1-Lipschitz: the same bound holds after it."""
    return (K * U * absprod) * SECOND_ORDER + 2.0 ** -8 * z.abs() + TINY


GELU_LIP = 1.13      # max |gelu'| (at z = sqrt(2): 1.1289)
ERF_ABS = 1.5e-6     # erf_exp (csrc/dct_common.h): Abramowitz-Stegun 7.1.26's 1.5e-7, five Horner roundings and
                     # v_rcp_f32's ulp on the polynomial (6e-7), v_exp_f32's ulp and its argument's three roundings
                     # (2e-7), the final subtraction (6e-8): 1.0e-6, taken as 1.5e-6


def gelu_ref(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_out_bound(z, absprod, K):
    """bf16 gelu(z) of the fp32 pre-activation: the accumulation and bias-add error of z through gelu's slope, the
    erf approximation (0.5 |z| ERF_ABS) and gelu_f's three products, and the bf16 rounding of the result."""
    ez = (K * U * absprod + 2 * U * z.abs()) * SECOND_ORDER
    return GELU_LIP * ez + 0.5 * z.abs() * ERF_ABS + (3 * U + 2.0 ** -8) * gelu_ref(z).abs() + TINY


def dw_slices(K, splits):
    """[k0, k1) of every split-K slice: ceil(nk / splits) k-tiles each, the last one what is left."""
    nk = K // GBK
    per = -(-nk // splits)
    return [(s * per * GBK, min(nk, (s + 1) * per) * GBK) for s in range(splits)]


# (M, N, K, splits, what) of dct_gemm_bf16_dw_partials_adam: dW [M][N] = dZ^T X, dZ [K][M], X [K][N].  All reach
# gemm2_kernel<true, false, true, 128, 2, 4> (r unset) / gemm2_dw_adam_kernel<S, F4> (r set).
DW_CASES = [
    (256, 128, 512, 4, "two row tiles, even slices of two k-tiles"),
    (200, 136, 448, 3, "ragged tiles in M and N; slices of 3, 3 and 1 k-tiles"),
    (128, 128, 64, 1, "one k-tile: a single LDS stage"),
    (128, 128, 512, 8, "8 slices of one k-tile"),
]
# rider of the test -> the kernel the launch reaches (S = 8 when a part range has more than 4 slices, else 4)
DW_KERNELS = {"none": "gemm2_kernel<true, false, true, 128, 2, 4>", "scalar": "gemm2_dw_adam_kernel<S, false>",
              "float4": "gemm2_dw_adam_kernel<S, true>"}
DW_REJECTED = [
    (128, 128, 64, 2, "splits > K / 64"),
    (128, 128, 384, 4, "(splits - 1) * ceil(nk / splits) >= nk: the last slice would be empty"),
]
# (n, parts case or None, f4, what) of the Adam range riding in the dW launch
RIDE_CASES = [
    (4099, "s234", 0, "gemm2_dw_adam_kernel<4, false>"),
    (4099, "s234", 1, "gemm2_dw_adam_kernel<4, true>"),
    (4099, "s148", 0, "gemm2_dw_adam_kernel<8, false>"),
    (4099, "s148", 1, "gemm2_dw_adam_kernel<8, true>"),
    (600000, None, 0, "gemm2_dw_adam_kernel<4, false>: more than one pass of 256 workgroups of 512 elements"),
]

EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_GELU, EPI_RELU_MASK, EPI_GELU_GRAD = 1, 2, 3, 4, 5
W8, W4 = "gemm2_gather_kernel<128, 2, 4, 128>", "gemm2_gather_kernel<128, 2, 2, 64>"


def gather_kernel(M, N, K, cus):
    """The kernel dct_gemm_bf16_gather_fwd launches on a device of ``cus`` compute units: 8 waves and 128-deep k
    stages for a grid between half a tile and one tile per unit, else 4 waves and 64-deep stages."""
    tiles = -(-M // 128) * -(-N // 128)
    return W8 if tiles <= cus and 2 * tiles > cus and K % 128 == 0 and K >= 256 else W4


# (M, N, K, kernel it is meant to reach, what)
GATHER_CASES = [
    (200, 264, 64, W4, "one k stage; three column tiles: a_out bands of 43 rows, no multiple of a pass's 32"),
    (200, 264, 192, W4, "three k stages"),
    (128, 8, 128, W4, "one narrow column tile: every row of a_out from one workgroup"),
    (2100, 1024, 256, W8, "136 tiles, two 128-deep stages"),
    (2100, 1024, 384, W8, "136 tiles, three 128-deep stages: a refilled LDS buffer"),
]
GATHER_REJECTED = [
    (128, 12, 64, EPI_BIAS, 4, "N % 8 != 0"),
    (128, 8, 96, EPI_BIAS, 4, "K % 64 != 0"),
    (128, 8, 64, EPI_BIAS, 5, "nz = 5"),
    (128, 8, 64, EPI_RELU_MASK, 4, "the ReLU-mask epilogue"),
    (128, 8, 64, EPI_GELU_GRAD, 4, "the GELU' epilogue"),
]
LDX_PAD = 8  # the padded dataset's row stride is K + 8


def batch_geometry(M):
    """(stride, n_items, idx entries, cursors): cursor 0 lies inside the list; at cursor 2 the second half of the batch
    wraps.  The index buffer holds 3 M valid entries, so a gather that forgot to wrap reads the wrong rows, not
    past the buffer."""
    return M, 2 * M + M // 2, 3 * M, (0, 2)


def gather_inputs(M, N, K, seed):
    """Dataset X [rows][K + 8] bf16 (pad columns NaN), W [N][K] bf16 ~ 1 / sqrt(K), bias, labels, and two index lists
    of 3 M entries: a permutation and one with repeated rows."""
    gen = torch.Generator().manual_seed(seed)
    rows = 3 * M + 7
    X = torch.full((rows, K + LDX_PAD), float("nan"))
    X[:, :K] = torch.randn(rows, K, generator=gen)
    W = torch.randn(N, K, generator=gen) / math.sqrt(K)
    bias = torch.randn(N, generator=gen) * 0.5
    Y = torch.randint(0, 1000, (rows,), generator=gen, dtype=torch.int32)
    perm = torch.randperm(rows, generator=gen)[:3 * M].to(torch.int32)
    rep = torch.randint(0, max(1, M // 4), (3 * M,), generator=gen, dtype=torch.int32)
    return X.to(torch.bfloat16), W.to(torch.bfloat16), bias.float(), Y, {"permutation": perm, "repeated": rep}


# (B, row bytes) of the batch-gather launches; the cursors and index lists are batch_geometry's
STEP_CASES = [(B, rb) for B in (1, 50, 4096) for rb in (16, 512)]
ZERO_NS = [1, 3, 4, 5, (1 << 20) | 3]
# launcher -> the kernel it reaches (csrc/step_kernels.hip)
STEP_LAUNCHERS = {
    "gather_batch_step_ranges": "gather_batch_kernel",
    "zero_f32": "gather_batch_kernel (B = 0, one zero range)",
    "ag_step_prologue": "ag_prologue_kernel",
    "step_end": "step_end_kernel",
}
