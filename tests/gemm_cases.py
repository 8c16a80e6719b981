"""The bf16 GEMM launchers of csrc/gemm_bf16.hip (dct_gemm_bf16, _ex, _bt, _residual) and dct_bias_act_bwd as tables of
cases: which kernel a launch reaches, fp64 references of the same bf16 / fp32 inputs, and error bounds derived from the
roundings the kernels perform.  tests/test_gemm_cases_cpu.py runs a torch fp32 / bf16 emulation of the kernels (and a
list of mutants) against the bounds and checks the tables' coverage; tests/test_gemm_kernels_gpu.py launches them.

Conventions (wide_step_cases / tt_cases): u = 2^-24 per fp32 rounding, BF = 2^-8 relative per bf16 rounding, an MFMA
accumulation of K products costs K u sum|a||b| whatever the order, a hardware transcendental HW (inside
tt_cases.gelu_grad_bound and wide_step_cases.gelu_out_bound, which this module takes as they are).

A plain module, not a conftest: the tests import it."""
import functools
import math
from collections import namedtuple

import torch

from tt_cases import BF, gelu_grad_bound, gelu_grad_ref, ratio  # noqa: F401  (the tests take ratio from here)
from wide_step_cases import SECOND_ORDER, TINY, U, fwd_bound, gelu_out_bound, gelu_ref, gemm_ref, partial_bound

EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_GELU, EPI_RELU_MASK, EPI_GELU_GRAD = range(6)
EPI_NAMES = ("none", "bias", "bias_relu", "bias_gelu", "relu_mask", "gelu_grad")
GBK = 64
INPUT_SETS = ("unit", "edge")
PAD = 8                      # padded leading dimensions are ld + 8
MIN_BF16 = 2.0 ** -133       # the smallest positive bf16 (subnormal): a ReLU output the mask must still pass


# ------------------------------------------------------------------------------------------------ dispatch mirror
def v2_ok(M, N, K, ta, tb, lda, ldb, aligned=True, epi_aligned=True):
    """gemm_v2_ok: the LDS-DMA kernels take K % 64 == 0, 16-byte aligned A and B with lda, ldb % 8 == 0, 8-row chunks
    of a k-major image inside the operand (ta: M % 8 == 0, !tb: N % 8 == 0), and 16-byte aligned bias / residual
    (their float4 reads in the epilogue)."""
    if K % GBK or not aligned or lda % 8 or ldb % 8 or not epi_aligned:
        return False
    if ta and M % 8:
        return False
    if not tb and N % 8:
        return False
    return True


def gemm_kernel(M, N, K, ta, tb, out_f32, epilogue, residual, accumulate, lda, ldb, aligned, cus, epi_aligned=True):
    """(kernel name, splits) a dct_gemm_bf16 / _ex / _residual launch reaches on a device of ``cus`` compute units:
    the mirror of gemm_v2_ok and launch_gemm2.  ``accumulate`` changes what the split kernels add into (and whether
    the atomic form clears C first), not which kernel runs."""
    if not v2_ok(M, N, K, ta, tb, lda, ldb, aligned, epi_aligned):
        return "generic<%d,%d>" % (ta, tb), 1
    tiles_n = -(-N // 128)
    tiles = -(-M // 128) * tiles_n
    nk = K // GBK
    splits = 1
    if out_f32 and epilogue == EPI_NONE and not residual and tiles < 256 and nk >= 8:
        splits = max(1, min(nk // 8, -(-cus // tiles)))
    if splits == 1 and tiles <= cus and 2 * tiles > cus and K % 128 == 0 and K >= 256:
        return "k128<%d,%d>" % (ta, tb), 1
    if not ta and splits == 1 and (nk <= 4 or tiles <= cus) and tiles < 1024:
        return "bm64<%d>" % tb, 1
    if splits > 1:
        # split_partials: the two-pass buffer serves up to 4 slices (outside stream capture, as every test is)
        return ("split2pass<%d,%d>" if splits <= 4 else "splitatomic<%d,%d>") % (ta, tb), splits
    return "tile128<%d,%d>" % (ta, tb), 1


def reduce_variant(N):
    """splitk_reduce_kernel: four columns per thread when N % 4 == 0, else one element per thread."""
    return "float4" if N % 4 == 0 else "scalar"


def slices(K, splits):
    """[k0, k1) of every split-K slice of launch_gemm2: ceil(nk / splits) k-tiles each, the last what is left."""
    nk = K // GBK
    per = -(-nk // splits)
    return [(min(nk, s * per) * GBK, min(nk, (s + 1) * per) * GBK) for s in range(splits)]


ALL_KERNELS = (["generic<%d,%d>" % (a, b) for a in (0, 1) for b in (0, 1)] + ["bm64<0>", "bm64<1>"] +
               ["%s<%d,%d>" % (k, a, b) for k in ("k128", "split2pass", "splitatomic", "tile128")
                for a in (0, 1) for b in (0, 1)])
# tile128 without TA needs > 256 tiles and > 4 k-tiles; the case table holds it for NT (the forward) and NN (dX)

# ------------------------------------------------------------------------------------------------ cases
# name, M, N, K, ta, tb, lda_pad / ldb_pad (0 or PAD; "odd": lda = K + 4; "unaligned": A two bytes past a 16-byte
# boundary), the kernel the plain bf16-out launch is meant to reach at 256 CUs, the variants it runs, what it is for
Case = namedtuple("Case", "name M N K ta tb ld kernel variants what")
Variant = namedtuple("Variant", "name entry epi out_f32 acc ldc_pad colsum")

V = Variant
FWD = [V("none_bf16", "gemm", EPI_NONE, 0, 0, 0, 0), V("bias_f32_acc_ldc", "gemm", EPI_BIAS, 1, 1, PAD, 0),
       V("relu_bf16_ldc", "gemm", EPI_BIAS_RELU, 0, 0, PAD, 0), V("gelu_bf16_aux", "gemm", EPI_BIAS_GELU, 0, 0, 0, 0),
       V("gelu_bf16_aux_ldc", "gemm", EPI_BIAS_GELU, 0, 0, PAD, 0), V("bias_bf16_acc", "gemm", EPI_BIAS, 0, 1, 0, 0)]
BWD = [V("mask_bf16_acc_ldc", "gemm", EPI_RELU_MASK, 0, 1, PAD, 0), V("mask_f32", "gemm", EPI_RELU_MASK, 1, 0, 0, 0),
       V("gelugrad_bf16", "gemm", EPI_GELU_GRAD, 0, 0, 0, 0), V("gelugrad_f32_ldc", "gemm", EPI_GELU_GRAD, 1, 0, PAD, 0)]
CS = [V("colsum_bf16", "ex", EPI_NONE, 0, 0, 0, 1), V("colsum_bias_f32_acc", "ex", EPI_BIAS, 1, 1, PAD, 1)]
ALLV = FWD + BWD + CS
SPLITV = [V("split", "gemm", EPI_NONE, 1, 0, 0, 0), V("split_acc_ldc", "gemm", EPI_NONE, 1, 1, PAD, 0),
          V("split_colsum", "ex", EPI_NONE, 1, 0, PAD, 1), V("split_colsum_acc", "ex", EPI_NONE, 1, 1, 0, 1)]
BT = [V("bt_relu", "bt", EPI_BIAS_RELU, 0, 0, 0, 0), V("bt_gelu_ldc", "bt", EPI_BIAS_GELU, 0, 0, PAD, 0),
      V("bt_bias_f32", "bt", EPI_BIAS, 1, 0, PAD, 0)]
RES = [V("residual_bias", "residual", EPI_BIAS, 1, 0, 0, 0), V("residual", "residual", EPI_NONE, 1, 0, 0, 0)]
GENV = [FWD[0], FWD[1], FWD[3], BWD[0], BWD[3]]

CASES = [
    Case("bm64_nt_1", 200, 136, 64, 0, 1, PAD, "bm64<1>", ALLV, "one k stage, ragged tiles in M and N"),
    Case("bm64_nn_1", 200, 136, 64, 0, 0, PAD, "bm64<0>", ALLV, "one k stage, k-major B image"),
    Case("bm64_nt_3", 200, 136, 192, 0, 1, 0, "bm64<1>", FWD + CS, "three k stages"),
    Case("bm64_nn_3", 200, 136, 192, 0, 0, 0, "bm64<0>", BWD + CS, "three k stages"),
    Case("bm64_nt_5", 200, 136, 320, 0, 1, PAD, "bm64<1>", FWD + BWD, "five k stages: an LDS buffer is refilled"),
    Case("bm64_nn_5", 200, 136, 320, 0, 0, PAD, "bm64<0>", FWD + BWD, "five k stages: an LDS buffer is refilled"),
    Case("tile128_tn_1", 136, 128, 64, 1, 0, PAD, "tile128<1,0>", ALLV, "k-major A image, one stage"),
    Case("tile128_tt_1", 136, 128, 64, 1, 1, PAD, "tile128<1,1>", ALLV, "k-major A image, one stage"),
    Case("tile128_tn_5", 136, 128, 320, 1, 0, 0, "tile128<1,0>", FWD + BWD, "five stages"),
    Case("tile128_tt_5", 136, 128, 320, 1, 1, 0, "tile128<1,1>", FWD + BWD, "five stages"),
    Case("tile128_nt_big", 2170, 2048, 320, 0, 1, 0, "tile128<0,1>", [FWD[2]],
         "272 tiles > 256 CUs and 5 k-tiles, ragged last row tile: the largest case"),
    Case("tile128_nn_big", 2170, 2048, 320, 0, 0, 0, "tile128<0,0>", [BWD[0], BWD[2]], "the same through the k-major B image"),
    Case("k128_nt_2", 1096, 1920, 256, 0, 1, 0, "k128<0,1>", [FWD[2], FWD[3], FWD[5], CS[0]], "135 tiles, two 128-deep stages"),
    Case("k128_nn_3", 1096, 1920, 384, 0, 0, 0, "k128<0,0>", [BWD[0], BWD[2]], "135 tiles, three stages: a refill"),
    Case("k128_tn_3", 1096, 1920, 384, 1, 0, 0, "k128<1,0>", [FWD[1], CS[0]], "three stages, k-major A and B"),
    Case("k128_tt_2", 1096, 1920, 256, 1, 1, 0, "k128<1,1>", [FWD[0], BWD[3], FWD[5]], "two stages, k-major A"),
    Case("k128_nt_3", 1096, 1920, 384, 0, 1, PAD, "k128<0,1>", [FWD[4]], "three stages, padded lda / ldb"),
    Case("k128_nn_2", 1096, 1920, 256, 0, 0, 0, "k128<0,0>", [BWD[3]], "two stages, k-major B"),
    Case("k128_tn_2", 1096, 1920, 256, 1, 0, PAD, "k128<1,0>", [FWD[2]], "two stages, k-major A and B, padded lda / ldb"),
    Case("k128_tt_3", 1096, 1920, 384, 1, 1, 0, "k128<1,1>", [BWD[0]], "three stages: a refill, k-major A"),
    Case("split2_tn_2", 256, 200, 1024, 1, 0, 0, "split2pass<1,0>", SPLITV, "the dW form, 2 slices of 8 k-tiles"),
    Case("split2_nt_2", 256, 200, 1024, 0, 1, PAD, "split2pass<0,1>", SPLITV, "2 slices of 8 k-tiles"),
    Case("split2_tn_uneven", 256, 200, 1088, 1, 0, PAD, "split2pass<1,0>", SPLITV, "slices of 9 and 8 k-tiles"),
    Case("split2_nt_uneven", 256, 200, 1088, 0, 1, 0, "split2pass<0,1>", SPLITV, "slices of 9 and 8 k-tiles"),
    Case("split2_tn_4", 200, 72, 2048, 1, 0, 0, "split2pass<1,0>", SPLITV, "4 slices, one column tile"),
    Case("split2_nn_4", 200, 72, 2048, 0, 0, 0, "split2pass<0,0>", SPLITV[:2], "4 slices, NN"),
    Case("split2_tt_4", 200, 70, 2048, 1, 1, 0, "split2pass<1,1>", SPLITV[:2], "N % 4 != 0: the reduce's scalar form"),
    Case("split2_nt_scalar", 136, 70, 1024, 0, 1, 0, "split2pass<0,1>", SPLITV, "N % 4 != 0: the reduce's scalar form"),
    Case("atomic_tn_5", 136, 40, 2560, 1, 0, 0, "splitatomic<1,0>", SPLITV, "5 slices of 8 k-tiles, atomics"),
    Case("atomic_nt_5", 136, 40, 2560, 0, 1, PAD, "splitatomic<0,1>", SPLITV, "5 slices, atomics"),
    Case("atomic_nn_5", 136, 40, 2560, 0, 0, 0, "splitatomic<0,0>", SPLITV[:2], "5 slices, atomics"),
    Case("atomic_tt_5", 136, 40, 2560, 1, 1, 0, "splitatomic<1,1>", SPLITV[:2], "5 slices, atomics"),
    Case("gen_k72_nt", 200, 136, 72, 0, 1, 0, "generic<0,1>", GENV, "K % 64 != 0: two k-tiles, the second 8 wide"),
    Case("gen_k600_nn", 130, 72, 600, 0, 0, 0, "generic<0,0>", GENV, "K % 64 != 0, ten k-tiles"),
    Case("gen_k72_tn", 136, 72, 72, 1, 0, 0, "generic<1,0>", GENV + [CS[1]], "K % 64 != 0; colsum by the column kernel"),
    Case("gen_k600_tt", 136, 72, 600, 1, 1, 0, "generic<1,1>", GENV + [CS[0]], "K % 64 != 0; colsum by the column kernel"),
    Case("gen_m_tn", 133, 72, 64, 1, 0, 0, "generic<1,0>", GENV + [CS[0]], "ta with M % 8 != 0 (lda = M: scalar staging)"),
    Case("gen_m_tt", 133, 72, 128, 1, 1, 0, "generic<1,1>", GENV, "ta with M % 8 != 0"),
    Case("gen_n_nn", 130, 70, 64, 0, 0, 0, "generic<0,0>", GENV, "!tb with N % 8 != 0 (ldb = N: scalar staging)"),
    Case("gen_n_tn", 136, 70, 128, 1, 0, 0, "generic<1,0>", GENV, "!tb with N % 8 != 0"),
    Case("gen_lda_nt", 130, 72, 64, 0, 1, "odd", "generic<0,1>", GENV, "lda % 8 != 0 (lda = K + 4)"),
    Case("gen_unaligned_nt", 130, 72, 128, 0, 1, "unaligned", "generic<0,1>", GENV, "A 2-byte but not 16-byte aligned"),
    Case("gen_m1_nt", 1, 72, 72, 0, 1, 0, "generic<0,1>", GENV, "M = 1"),
    Case("gen_n3_nt", 130, 3, 72, 0, 1, 0, "generic<0,1>", GENV, "N = 3"),
    Case("bm64_m1_nt", 1, 136, 64, 0, 1, 0, "bm64<1>", FWD, "M = 1 on the LDS-DMA kernel: every A row clamps to row 0"),
    Case("bm64_n3_nt", 130, 3, 64, 0, 1, 0, "bm64<1>", FWD[:3], "N = 3 on the LDS-DMA kernel: scalar epilogue"),
    # dct_gemm_bf16_bt: N = 264, a ragged column tile with N % 8 == 0
    Case("bt_bm64", 200, 264, 192, 0, 1, PAD, "bm64<1>", BT, "W^T out of the half-height kernel"),
    Case("bt_k128", 5500, 264, 384, 0, 1, 0, "k128<0,1>", BT,
         "43 x 3 = 129 tiles: W^T out of the 8-wave kernel, 32 k rows per pass, its last column tile 8 wide"),
    Case("bt_k128_2", 5500, 264, 256, 0, 1, PAD, "k128<0,1>", BT[:2], "the same with two stages and padded lda / ldb"),
    Case("bt_tile128", 2100, 2056, 320, 0, 1, 0, "tile128<0,1>", BT[:2], "W^T out of the plain kernel, ragged N tile"),
    # dct_gemm_bf16_residual
    Case("res_v2", 200, 136, 192, 0, 1, 0, "bm64<1>", RES, "residual on the LDS-DMA kernel"),
    Case("res_v2_split_shape", 256, 200, 1024, 0, 1, 0, "bm64<1>", RES, "a split-K shape: never split with a residual"),
    Case("res_generic", 130, 72, 72, 0, 1, 0, "generic<0,1>", RES, "residual on the generic kernel"),
]
CASE = {c.name: c for c in CASES}
BIG = {"tile128_nt_big", "tile128_nn_big", "bt_tile128"}  # one input set only: 4.4 M outputs each

# dct_gemm_bf16_bt refusals (nothing launched): (what, overrides)
BT_REJECTED = [
    ("fp32 out with EPI_NONE could split", dict(out_f32=1, epi=EPI_NONE)),
    ("N % 8 != 0", dict(N=260)),
    ("bt_ld % 8 != 0", dict(bt_ld_extra=4)),
    ("bt_out not 16-byte aligned", dict(bt_shift=1)),
    ("K % 64 != 0", dict(K=200)),
    ("bias not 16-byte aligned", dict(bias_shift=1)),
]
# dct_gemm_bf16_ex with colsum on the generic path without trans_a: hipErrorNotSupported, nothing launched
EX_REJECTED = [("gen_k72_nt", "NT"), ("gen_k600_nn", "NN")]
# a bias 4 bytes past a 16-byte boundary: the launcher takes the generic kernel (scalar bias reads), same result
UNALIGNED_BIAS = ("bm64_nt_1", FWD[1], "generic<0,1>")
# the same for the residual of dct_gemm_bf16_residual
UNALIGNED_RESIDUAL = ("res_v2", RES[0], "generic<0,1>")


def leading(case):
    """(lda, ldb, A shift in elements) of the stored operands: A [M][lda] or, ta, [K][lda]; B [N][ldb] (tb) or [K][ldb]."""
    a_cols = case.M if case.ta else case.K
    b_cols = case.K if case.tb else case.N
    if case.ld == "odd":
        return a_cols + 4, b_cols, 0
    if case.ld == "unaligned":
        return a_cols, b_cols, 1
    return a_cols + case.ld, b_cols + case.ld, 0


def kernel_of(case, v, cus, epi_aligned=True):
    lda, ldb, shift = leading(case)
    return gemm_kernel(case.M, case.N, case.K, case.ta, case.tb, v.out_f32, v.epi, v.entry == "residual", v.acc,
                       lda, ldb, shift == 0, cus, epi_aligned)


# ------------------------------------------------------------------------------------------------ inputs
def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


@functools.lru_cache(maxsize=8)
def problem(name, kind):
    """Logical operands a [M][K], b [K][N] (bf16), bias, the two aux tensors, C0, residual, colsum0 and the fp64
    product.  unit: a ~ N(0, 1), b ~ N(0, 1 / K), tabular scale.  edge: a zero row of a and a zero column of b (exact
    zeros out), two k columns of a at +-64 meeting equal rows of b (they cancel exactly and quadruple sum|a||b|), and
    b scaled by 2^-6 so the product sits far below bias, C0 and the residual."""
    c = CASE[name]
    g = torch.Generator().manual_seed(_seed(name) + (7 if kind == "edge" else 0))
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    M, N, K = c.M, c.N, c.K
    a, b = r(M, K), r(K, N) / math.sqrt(K)
    if kind == "edge":
        b = b * 2.0 ** -6
        b[:, N // 3] = 0.0
        b[K - 2] = b[1]
        a[:, 1], a[:, K - 2] = 64.0, -64.0
        a[M // 2] = 0.0
    a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
    bias = r(N) * 0.5
    pre = (r(M, N) * 1.5).to(torch.bfloat16)          # GELU' aux: pre-activations
    act = torch.relu(r(M, N))                          # ReLU-mask aux: about half exact zeros
    u = torch.rand(M, N, generator=g)
    act = torch.where(u < 0.1, torch.full_like(act, -0.0), act)
    act = torch.where((u >= 0.1) & (u < 0.2), torch.full_like(act, MIN_BF16), act).to(torch.bfloat16)
    z, absprod = gemm_ref(a, b)
    scale = 0.2 * float(absprod.mean())
    c0 = r(M, N) * 0.5 * min(1.0, scale)
    p = dict(a=a, b=b, bias=bias, pre=pre, act=act, c0=c0, c0_bf16=c0.to(torch.bfloat16), res=r(M, N) * 0.7,
             cs0=r(M), z=z, absprod=absprod, M=M, N=N, K=K)
    return p


# ------------------------------------------------------------------------------------------------ references
def expect(p, v, splits=1, with_bias=True, colsum_adds=1):
    """{tensor: (fp64 reference, bound)} of one launch.

    t = a b (+ bias) (+ residual) is accumulated in fp32: K u sum|a||b| whatever the order (for a split launch the
    slices' K / S steps each and the S additions of the reduce pass or the atomics fit the same K u sum|a||b|:
    K / S + S <= K), and u of the sum of magnitudes for each of the bias and residual additions.
      none / bias / bias_relu: v = t, ReLU is 1-Lipschitz.
      bias_gelu: aux = bf16(t) (BF |t|); v = gelu_f(t): wide_step_cases.gelu_out_bound (bf16 out only).
      relu_mask: v = t where aux > 0, else exactly 0 (-0.0 and 0.0 fail the mask, the smallest subnormal passes).
      gelu_grad: v = t g'(aux): |t| gelu_grad_bound + |g'| e_t + u |v|.
    The output: fp32 stores v, or C0 + v (u (|C0| + |result|)); bf16 the same in fp32 (C0 widened exactly), then one
    bf16 rounding BF |result| of the result and of its error.  Split launches round the reduced sum once (u |result|)
    and, accumulating, once more into C0.  The atomic form adds its S partials into C0 one by one; each of those
    roundings is u of at most |C0| + sum|a||b|, which K u sum|a||b| still holds because the inputs keep
    |C0| <= sum|a||b| wherever a partial is not zero (test_atomic_accumulate_precondition)."""
    z, absprod, K = p["z"], p["absprod"], p["K"]
    out = {}
    mag = z.abs()
    t = z
    adds = 0
    if v.epi in (EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_GELU) and with_bias:
        t = t + p["bias"].double()
        mag = mag + p["bias"].double().abs()
        adds += 1
    if v.entry == "residual":
        t = t + p["res"].double()
        mag = mag + p["res"].double().abs()
        adds += 1
    e_t = (K * U * absprod + (adds + 1) * U * mag) * SECOND_ORDER
    if v.epi == EPI_BIAS_RELU:
        val, e_v = t.clamp_min(0.0), e_t
    elif v.epi == EPI_BIAS_GELU:
        out["aux"] = (t, fwd_bound(t, absprod, K) + adds * U * mag)
        val = gelu_ref(t)
        e_v = gelu_out_bound(t, absprod, K) + 1.13 * adds * U * mag - BF * val.abs()
    elif v.epi == EPI_RELU_MASK:
        keep = p["act"].double() > 0
        val, e_v = torch.where(keep, t, torch.zeros_like(t)), torch.where(keep, e_t, torch.zeros_like(t))
    elif v.epi == EPI_GELU_GRAD:
        x = p["pre"].double()
        gp = gelu_grad_ref(x)
        val = t * gp
        e_v = t.abs() * gelu_grad_bound(x) + gp.abs() * e_t + U * val.abs()
    else:
        val, e_v = t, e_t
    if splits > 1:
        e_v = partial_bound(val, absprod, K)
    if v.acc:
        c0 = (p["c0"] if v.out_f32 else p["c0_bf16"]).double()
        res = c0 + val
        e = e_v + U * (c0.abs() + res.abs())
    else:
        res, e = val, e_v + (0.0 if splits > 1 else U * val.abs())
    if not v.out_f32:
        e = e * (1 + BF) + BF * res.abs()
    out["C"] = (res, e + TINY)
    if v.colsum:
        out["colsum"] = colsum_expect(p, colsum_adds)
    return out


def colsum_expect(p, adds):
    """colsum[m] += sum_k op(A)[m][k]: K fp32 additions of exact bf16 values in some order, then ``adds`` atomic
    additions into the running vector (one per split slice, or per 64-row block of the column-sum kernel)."""
    a = p["a"].double()
    s, sa = a.sum(1), a.abs().sum(1)
    c0 = p["cs0"].double()
    ref = c0 + s
    return ref, ((p["K"] + adds) * U * (sa + c0.abs()) + U * ref.abs()) * SECOND_ORDER + TINY


# ------------------------------------------------------------------------------------------------ emulation
def _gelu32(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.70710678118654752))


def _gelu_grad32(z):
    return 0.5 * (1.0 + torch.erf(z * 0.70710678118654752)) + z * 0.3989422804014327 * torch.exp(-0.5 * z * z)


GEMM_MUTANTS = {
    "k_element_dropped": "C", "split_last_ktile_dropped": "C", "split_slice_missing": "C", "bias_of_next_column": "C",
    "bias_after_relu": "C", "mask_ge_zero": "C", "mask_row_stride_n": "C", "residual_omitted": "C",
    "accumulate_overwrites": "C", "colsum_wrong_axis": "colsum", "tile_16x16_transposed": "C",
}
# mutant -> (case, variant name) meant to catch it
MUTANT_CASES = {
    "k_element_dropped": [("bm64_nt_5", "none_bf16"), ("k128_nt_2", "relu_bf16_ldc"), ("gen_k600_nn", "none_bf16")],
    "split_last_ktile_dropped": [("split2_tn_uneven", "split"), ("atomic_tn_5", "split")],
    "split_slice_missing": [("split2_tn_4", "split"), ("atomic_nt_5", "split_acc_ldc")],
    "bias_of_next_column": [("bm64_nt_1", "relu_bf16_ldc"), ("bm64_nt_1", "bias_f32_acc_ldc")],
    "bias_after_relu": [("bm64_nt_3", "relu_bf16_ldc")],
    "mask_ge_zero": [("bm64_nn_1", "mask_f32"), ("tile128_tn_5", "mask_bf16_acc_ldc")],
    "mask_row_stride_n": [("bm64_nn_3", "mask_bf16_acc_ldc")],
    "residual_omitted": [("res_v2", "residual_bias"), ("res_generic", "residual")],
    "accumulate_overwrites": [("bm64_nt_1", "bias_f32_acc_ldc"), ("split2_nt_2", "split_acc_ldc"),
                              ("bm64_nn_1", "mask_bf16_acc_ldc")],
    "colsum_wrong_axis": [("tile128_tn_1", "colsum_bf16"), ("split2_tn_2", "split_colsum")],
    "tile_16x16_transposed": [("bm64_nt_1", "none_bf16"), ("tile128_tt_1", "gelu_bf16_aux")],
}


def emulate(p, v, splits=1, mutant=None):
    """The launch in torch at the kernel's precision: fp32 accumulation (per slice, then the slices in order), the
    epilogue in fp32, bf16 roundings where the kernel rounds.  ``mutant``: one of GEMM_MUTANTS."""
    a, b = p["a"].float(), p["b"].float()
    M, N, K = p["M"], p["N"], p["K"]
    if mutant == "k_element_dropped":
        a = a.clone()
        a[:, K // 2] = 0.0
    acc = torch.zeros(M, N)
    sl = slices(K, splits)
    for i, (k0, k1) in enumerate(sl):
        if mutant == "split_slice_missing" and i == len(sl) - 1:
            continue
        if mutant == "split_last_ktile_dropped" and i == 0:
            k1 -= GBK
        acc = acc + a[:, k0:k1] @ b[k0:k1]
    if K % GBK or splits == 1:
        acc = a @ b
    t = acc
    bias_epi = v.epi in (EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_GELU)
    bias = p["bias"].roll(-1) if mutant == "bias_of_next_column" else p["bias"]
    if bias_epi and mutant != "bias_after_relu":
        t = t + bias
    if v.entry == "residual" and mutant != "residual_omitted":
        t = t + p["res"]
    out = {}
    if v.epi == EPI_BIAS_RELU:
        t = t.clamp_min(0.0)
        if mutant == "bias_after_relu":
            t = t + bias
    elif v.epi == EPI_BIAS_GELU:
        out["aux"] = t.to(torch.bfloat16)
        t = _gelu32(t)
    elif v.epi == EPI_RELU_MASK:
        act = p["act"].float()
        if mutant == "mask_row_stride_n" and v.ldc_pad:
            padded = torch.ones(M, N + v.ldc_pad)
            padded[:, :N] = act
            act = padded.reshape(-1)[:M * N].reshape(M, N)
        t = torch.where((act >= 0) if mutant == "mask_ge_zero" else (act > 0), t, torch.zeros_like(t))
    elif v.epi == EPI_GELU_GRAD:
        t = t * _gelu_grad32(p["pre"].float())
    if v.acc and mutant != "accumulate_overwrites":
        t = t + (p["c0"] if v.out_f32 else p["c0_bf16"].float())
    if mutant == "tile_16x16_transposed":
        t = t.clone()
        t[:16, :16] = t[:16, :16].t().clone()
    out["C"] = t if v.out_f32 else t.to(torch.bfloat16)
    if v.colsum:
        s = p["a"].float().sum(1)
        if mutant == "colsum_wrong_axis":
            w = p["a"].float().sum(0)
            n = min(M, K)
            s = s.clone()
            s[:n] = w[:n]
        out["colsum"] = p["cs0"] + s
    return out


# ------------------------------------------------------------------------------------------------ dct_bias_act_bwd
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
# (M, N, ld pad, A shift): N % 8 != 0 and a shifted pointer reach bias_act_bwd_kernel<false>, the rest <true>
BAB_SHAPES = ([(M, N, 0, 0) for N in (8, 136, 1001) for M in (1, 64, 65, 333)] +
              [(M, N, PAD, 0) for N in (8, 136) for M in (65, 333)] + [(65, 136, 0, 1), (333, 8, 0, 1)])


def bab_kernel(M, N, ld, shift):
    return "bias_act_bwd_kernel<%s>" % ("true" if N % 8 == 0 and ld % 8 == 0 and shift == 0 else "false")


def bab_row_blocks(M, N):
    """gridDim.y of the launch: 64-row blocks, capped at max(64, 512 / column blocks)."""
    ncb = -(-(-(-N // 8)) // 64)
    return max(1, min(-(-M // 64), max(64, 512 // max(1, ncb))))


@functools.lru_cache(maxsize=4)
def bab_problem(M, N, act):
    g = torch.Generator().manual_seed(1000 * M + N + act)
    dy = torch.randn(M, N, generator=g).to(torch.bfloat16)
    pre = (torch.randn(M, N, generator=g) * 1.5).to(torch.bfloat16)
    aux = torch.relu(pre.float()).to(torch.bfloat16) if act == ACT_RELU else pre
    if act == ACT_RELU and M * N > 4:
        aux.view(-1)[1] = -0.0
        aux.view(-1)[2] = MIN_BF16
    return dict(dy=dy, aux=aux, db0=torch.randn(N, generator=g) * 3.0)


def bab_expect(p, act, accumulate):
    """dZ = bf16(dY act'(aux)): exact for NONE and RELU (a bf16 value or zero), |dY| gelu_grad_bound + u |d| and the
    bf16 rounding for GELU.  dbias (+)= the column sums of the UNROUNDED fp32 d: M additions in some order (4 row
    lanes, then atomics over the row blocks) of terms each known to e_d, into dbias0 when accumulating."""
    dy, x = p["dy"].double(), p["aux"].double()
    M = dy.shape[0]
    if act == ACT_RELU:
        d, e_d = torch.where(x > 0, dy, torch.zeros_like(dy)), torch.zeros_like(dy)
    elif act == ACT_GELU:
        gp = gelu_grad_ref(x)
        d = dy * gp
        e_d = dy.abs() * gelu_grad_bound(x) + U * d.abs()
    else:
        d, e_d = dy, torch.zeros_like(dy)
    dz = (d, e_d * (1 + BF) + (BF * d.abs() if act == ACT_GELU else 0.0) + TINY)
    c0 = p["db0"].double() if accumulate else torch.zeros(dy.shape[1], dtype=torch.float64)
    s = c0 + d.sum(0)
    e_s = (e_d.sum(0) + (M + 1) * U * (d.abs().sum(0) + c0.abs()) + U * s.abs()) * SECOND_ORDER + TINY
    return dict(dZ=dz, dbias=(s, e_s))


def bab_emulate(p, act, accumulate, mutant=None):
    dy, x = p["dy"].float(), p["aux"].float()
    d = dy if act == ACT_NONE else torch.where(x > 0, dy, torch.zeros_like(dy)) if act == ACT_RELU \
        else dy * _gelu_grad32(x)
    s = d.sum(0)
    if mutant == "flag0_adds_to_dbias" or accumulate:
        s = p["db0"] + s
    return dict(dZ=d.to(torch.bfloat16), dbias=s)


def launch_plan(case, v, cus, epi_aligned=True):
    """(kernel, splits, atomic additions into each colsum element) of a variant's launch."""
    kernel, splits = kernel_of(case, v, cus, epi_aligned)
    adds = splits
    if kernel.startswith("generic"):
        adds = bab_row_blocks(case.K, case.M)  # dct_bias_act_bwd over A [K][M]
    return kernel, splits, adds
