"""dct_gemm_bf16, dct_gemm_bf16_ex, dct_gemm_bf16_bt, dct_gemm_bf16_residual and dct_bias_act_bwd, launch by launch and
element by element against the fp64 references and derived bounds of tests/gemm_cases.py.  Every comparison is kernel
against reference; the two places the source states bit-identity (two launches of the two-pass split-K, bt_out against
W^T) are asserted in addition.  Every output sits in a buffer with a guard row after it and guard fill in its padding
columns, operands carry NaN in theirs; outputs that must not be written (aux without GELU, C and colsum of a refused
launch, a null dZ) keep their fill.  Each test prints the CU count, the kernel the launch reaches on this device
(gemm_cases.gemm_kernel) and the worst error / bound per tensor before it asserts <= 1; a case whose kernel here differs
from the one it is meant for skips, and on a 256-CU device none may.

Found while writing these tests (fixed in the same change):
  - dct_bias_act_bwd(accumulate_bias = 0) added into whatever dbias held from M > 64 on (several row blocks per column
    add atomically): the launcher now clears dbias[0, N) first.  test_bias_act_bwd, flag 0 with M = 65 and 333.
  - dct_gemm_bf16_ex with colsum, trans_a = 0, on a shape the LDS-DMA kernels do not take wrote C and then returned
    hipErrorNotSupported: it now refuses before launching.  test_ex_colsum_refused_on_the_generic_path.
  - the LDS-DMA kernels read bias and residual as float4 whenever C, ldc and aux allow vector stores, but nothing checked
    their own alignment: gemm_v2_ok now sends such a launch to the generic kernel (scalar reads), and dct_gemm_bf16_bt
    refuses it.  test_unaligned_bias_takes_the_generic_kernel, test_unaligned_residual_takes_the_generic_kernel,
    test_bt_rejections.
  - dct_bias_act_bwd with RELU / GELU, and dct_gemm_bf16 / _ex / _bt with EPI_RELU_MASK / EPI_GELU_GRAD, would have read
    through a null aux: refused now.  test_bias_act_bwd_refuses_a_null_aux,
    test_null_aux_is_refused_by_the_epilogues_that_read_it.

Measured on an MI355X (256 CUs, 2026-10-21), worst error / bound over every case, variant and input set
(test_zz_report_worst_ratios prints them); no case skipped:

    launcher, kernel                     C bf16   C fp32   aux      colsum
    dct_gemm_bf16      generic           0.992    0.389    0.992
    dct_gemm_bf16      bm64              0.994    0.389    0.994
    dct_gemm_bf16      k128              0.995    0.403    0.995
    dct_gemm_bf16      tile128           0.994    0.388    0.994
    dct_gemm_bf16      split2pass                 0.0028
    dct_gemm_bf16      splitatomic                0.0005
    dct_gemm_bf16_ex   generic           0.985    0.323             0.0069
    dct_gemm_bf16_ex   bm64              0.993    0.389             0.0054
    dct_gemm_bf16_ex   k128              0.977                      0.0014
    dct_gemm_bf16_ex   tile128           0.987    0.388             0.0061
    dct_gemm_bf16_ex   split2pass                 0.0028            0.0002
    dct_gemm_bf16_ex   splitatomic                0.0005            0.0000
    dct_gemm_bf16_bt   bm64              0.989    0.031    0.989
    dct_gemm_bf16_bt   k128              0.994    0.015    0.994
    dct_gemm_bf16_bt   tile128           0.972             0.970
    dct_gemm_bf16_residual bm64 / generic         0.244 / 0.244
    dct_bias_act_bwd   dbias 0.333, dZ 0.000 (NONE, RELU: exact) / 0.995 (GELU: the bf16 rounding)

Every ratio above 0.9 is a bf16 output (C, the GELU aux or the GELU dZ): the bound is the rounding to bf16 itself,
2^-8 |value|, plus an fp32 accumulation term a hundred times smaller, and a value just above a power of two is rounded by
2^-8 / (1 + 2^-8) of itself - 0.996 of the bound.  The fp32 outputs of the same kernels sit at 0.4 and below.  The
split-K figures are small because the order-free bound K u sum|a||b| charges every product a rounding of the whole sum;
the CPU test shows a dropped k-tile, a missing slice and a dropped k element outside it all the same.  On the parent
commit test_bias_act_bwd fails at its first accumulate_bias = 0 launch with more than one row block (M = 65, N = 8:
dbias error 20765 x its bound; NaN with a NaN-filled dbias).
"""
import functools

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

FILL_F32, FILL_BF16 = 12345.0, -7.0
WORST = {}


def _nat():
    from dct_amd.ops._native import native

    return native()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=1)
def _cus():
    return int(_nat().device_cu_count())


def _ratio(launcher, what, tensor, got, want, bound):
    """Worst |got - want| / bound on the CPU in fp64; a non-finite output counts as inf."""
    r = G.ratio(got.detach().cpu(), want, bound)
    print("  %s %s: worst error / bound %.4f" % (what, tensor, r))
    key = (launcher, tensor)
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


class Buf:
    """A [rows][ld] matrix on the device inside a larger allocation: ``shift`` elements past a 16-byte boundary, pad
    columns and one guard row after the last row filled with ``fill``."""

    def __init__(self, mat, ld, fill, dtype, shift=0):
        rows, cols = mat.shape
        self.rows, self.cols, self.ld, self.fill = rows, cols, ld, fill
        self.flat = torch.full((shift + (rows + 1) * ld + 8,), fill, dtype=dtype)
        self.view(self.flat, shift)[:rows, :cols] = mat.to(dtype)
        self.flat = self.flat.to(_dev())
        self.shift = shift
        self.ptr = self.flat.data_ptr() + shift * self.flat.element_size()
        self.initial = self.flat.clone()

    def view(self, flat, shift):
        return flat[shift:shift + (self.rows + 1) * self.ld].view(self.rows + 1, self.ld)

    def data(self):
        return self.view(self.flat, self.shift)[:self.rows, :self.cols]

    def guards_intact(self):
        """Everything outside [rows][cols] still holds the fill (NaN fill: still NaN)."""
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        self.view(keep, self.shift)[:self.rows, :self.cols] = False
        g = self.flat[keep].float()
        return bool(torch.isnan(g).all()) if self.fill != self.fill else bool((g == self.fill).all())

    def untouched(self):
        a, b = self.flat, self.initial
        return bool(((a == b) | (torch.isnan(a.float()) & torch.isnan(b.float()))).all())


def _operands(case, p):
    lda, ldb, shift = G.leading(case)
    nan = float("nan")
    A = Buf(p["a"].t() if case.ta else p["a"], lda, nan, torch.bfloat16, shift)
    B = Buf(p["b"].t() if case.tb else p["b"], ldb, nan, torch.bfloat16)
    return A, B, lda, ldb


def _run_variant(nat, case, p, A, B, lda, ldb, v, kind, bias_shift=0, bt=None, res_shift=0):
    """One launch of variant v, every check on it.  Returns the C buffer."""
    M, N, K = case.M, case.N, case.K
    cus = _cus()
    kernel, splits, adds = G.launch_plan(case, v, cus, epi_aligned=bias_shift == 0 and res_shift == 0)
    what = "%s %s %s [%s, %d CUs]" % (case.name, kind, v.name, kernel, cus)
    ldc = N + v.ldc_pad
    f32 = bool(v.out_f32)
    c0 = (p["c0"] if f32 else p["c0_bf16"]) if v.acc else torch.full((M, N), FILL_F32 if f32 else FILL_BF16)
    C = Buf(c0, ldc, FILL_F32 if f32 else FILL_BF16, torch.float32 if f32 else torch.bfloat16)
    bias_epi = v.epi in (G.EPI_BIAS, G.EPI_BIAS_RELU, G.EPI_BIAS_GELU)
    bias = Buf(p["bias"].reshape(1, N), N, 0.0, torch.float32, bias_shift)
    reads_aux = v.epi in (G.EPI_RELU_MASK, G.EPI_GELU_GRAD)
    if reads_aux:
        aux = Buf(p["act"] if v.epi == G.EPI_RELU_MASK else p["pre"], ldc, float("nan"), torch.bfloat16)
    else:
        aux = Buf(torch.full((M, N), FILL_BF16), ldc, FILL_BF16, torch.bfloat16)
    cs = Buf(p["cs0"].reshape(1, M), M, FILL_F32, torch.float32) if v.colsum else None
    bp = bias.ptr if bias_epi else 0
    launcher = "dct_gemm_bf16"
    if v.entry == "gemm":
        nat.gemm_bf16(A.ptr, B.ptr, C.ptr, bp, M, N, K, lda, ldb, ldc, case.ta, case.tb, v.epi, v.out_f32, v.acc, aux.ptr,
                      _st())
    elif v.entry == "ex":
        launcher = "dct_gemm_bf16_ex"
        nat.gemm_bf16_ex(A.ptr, B.ptr, C.ptr, bp, M, N, K, lda, ldb, ldc, case.ta, case.tb, v.epi, v.out_f32, v.acc,
                         aux.ptr, cs.ptr, _st())
    elif v.entry == "bt":
        launcher = "dct_gemm_bf16_bt"
        nat.gemm_bf16_bt(A.ptr, B.ptr, C.ptr, bp, M, N, K, lda, ldb, ldc, v.epi, v.out_f32, aux.ptr, bt.ptr, bt.ld, _st())
    else:
        launcher = "dct_gemm_bf16_residual"
        res = Buf(p["res"], N, float("nan"), torch.float32, res_shift)
        nat.gemm_bf16_residual(A.ptr, B.ptr, C.ptr, bp, res.ptr, M, N, K, _st())
        torch.cuda.synchronize()
        assert res.untouched(), what + ": residual changed"
    torch.cuda.synchronize()
    launcher += " " + kernel.split("<")[0]
    want = G.expect(p, v, splits, colsum_adds=adds)
    rs = [_ratio(launcher, what, "C fp32" if f32 else "C bf16", C.data(), *want["C"])]
    assert C.guards_intact(), what + ": wrote outside C[M][N]"
    if v.epi == G.EPI_BIAS_GELU:
        rs.append(_ratio(launcher, what, "aux", aux.data(), *want["aux"]))
        assert aux.guards_intact(), what + ": wrote outside aux[M][N]"
    else:
        assert aux.untouched(), what + ": aux written without the GELU epilogue"
    if v.colsum:
        rs.append(_ratio(launcher, what, "colsum", cs.data().reshape(M), *want["colsum"]))
        assert cs.guards_intact(), what + ": wrote outside colsum[M]"
    assert A.untouched() and B.untouched() and bias.untouched(), what + ": an operand changed"
    assert max(rs) <= 1.0, (what, rs)
    return C


GEMM_CASES = [c.name for c in G.CASES if all(v.entry in ("gemm", "ex") for v in c.variants)]


def _skip_unless_meant(case):
    cus = _cus()
    for v in case.variants:
        k = G.kernel_of(case, v, cus)[0]
        if k != case.kernel:
            pytest.skip("%s %s reaches %s on %d CUs, the case is meant for %s" % (case.name, v.name, k, cus, case.kernel))


@pytest.mark.parametrize("name", GEMM_CASES)
def test_gemm_matches_fp64_elementwise(name):
    """dct_gemm_bf16 / _ex: every variant of the case on both input sets."""
    nat, case = _nat(), G.CASE[name]
    _skip_unless_meant(case)
    print("%s: %d CUs, meant for %s (%s)" % (name, _cus(), case.kernel, case.what))
    for kind in (("unit",) if name in G.BIG else G.INPUT_SETS):
        p = G.problem(name, kind)
        A, B, lda, ldb = _operands(case, p)
        for v in case.variants:
            C = _run_variant(nat, case, p, A, B, lda, ldb, v, kind)
            if case.kernel.startswith("split2pass"):
                # slices stored and summed in slice order: the same bits every launch
                C2 = _run_variant(nat, case, p, A, B, lda, ldb, v, kind)
                assert bool(torch.equal(C.flat.view(torch.int32), C2.flat.view(torch.int32))), name + ": two-pass bits differ"


@pytest.mark.parametrize("name", [c.name for c in G.CASES if c.variants[0].entry == "bt"])
def test_gemm_bt_matches_fp64_and_leaves_the_transpose(name):
    """dct_gemm_bf16_bt: C (and aux) as above; bt_out bit-equal to W^T, its padding and guard row intact."""
    nat, case = _nat(), G.CASE[name]
    _skip_unless_meant(case)
    print("%s: %d CUs, meant for %s (%s)" % (name, _cus(), case.kernel, case.what))
    for kind in (("unit",) if name in G.BIG else G.INPUT_SETS):
        p = G.problem(name, kind)
        A, B, lda, ldb = _operands(case, p)
        for v in case.variants:
            bt = Buf(torch.full((case.K, case.N), FILL_BF16), case.N + v.ldc_pad, FILL_BF16, torch.bfloat16)
            _run_variant(nat, case, p, A, B, lda, ldb, v, kind, bt=bt)
            got = bt.data().cpu().contiguous()
            assert bool(torch.equal(got.view(torch.int16), p["b"].contiguous().view(torch.int16))), name + ": bt_out != W^T"
            assert bt.guards_intact(), name + ": wrote outside bt_out[K][N]"


@pytest.mark.parametrize("name", [c.name for c in G.CASES if c.variants[0].entry == "residual"])
def test_gemm_residual_matches_fp64(name):
    nat, case = _nat(), G.CASE[name]
    _skip_unless_meant(case)
    print("%s: %d CUs, meant for %s (%s)" % (name, _cus(), case.kernel, case.what))
    for kind in G.INPUT_SETS:
        p = G.problem(name, kind)
        A, B, lda, ldb = _operands(case, p)
        for v in case.variants:
            _run_variant(nat, case, p, A, B, lda, ldb, v, kind)


def test_unaligned_bias_takes_the_generic_kernel():
    """A bias 4 bytes past a 16-byte boundary: the launcher leaves the LDS-DMA kernels (float4 bias reads) for the
    generic one, and the result is the same reference's."""
    name, v, kernel = G.UNALIGNED_BIAS
    nat, case = _nat(), G.CASE[name]
    assert G.kernel_of(case, v, _cus(), epi_aligned=False)[0] == kernel
    for kind in G.INPUT_SETS:
        p = G.problem(name, kind)
        A, B, lda, ldb = _operands(case, p)
        _run_variant(nat, case, p, A, B, lda, ldb, v, kind, bias_shift=1)


def test_unaligned_residual_takes_the_generic_kernel():
    """A residual 4 bytes past a 16-byte boundary (its float4 reads in the LDS-DMA epilogue): dct_gemm_bf16_residual
    takes the generic kernel, and the result is the same reference's."""
    name, v, kernel = G.UNALIGNED_RESIDUAL
    nat, case = _nat(), G.CASE[name]
    assert G.kernel_of(case, v, _cus(), epi_aligned=False)[0] == kernel
    for kind in G.INPUT_SETS:
        p = G.problem(name, kind)
        A, B, lda, ldb = _operands(case, p)
        _run_variant(nat, case, p, A, B, lda, ldb, v, kind, res_shift=1)


def test_bt_rejections():
    """Every condition dct_gemm_bf16_bt states: an error, nothing written."""
    nat, case = _nat(), G.CASE["bt_bm64"]
    p = G.problem("bt_bm64", "unit")
    for what, o in G.BT_REJECTED:
        M, N, K = case.M, o.get("N", case.N), o.get("K", case.K)
        A = Buf(p["a"], case.K + G.PAD, float("nan"), torch.bfloat16)
        B = Buf(p["b"].t(), case.K + G.PAD, float("nan"), torch.bfloat16)
        f32 = o.get("out_f32", 0)
        C = Buf(torch.full((M, case.N), FILL_F32), case.N, FILL_F32, torch.float32 if f32 else torch.bfloat16)
        aux = Buf(torch.full((M, case.N), FILL_BF16), case.N, FILL_BF16, torch.bfloat16)
        bias = Buf(p["bias"].reshape(1, case.N), case.N, 0.0, torch.float32, o.get("bias_shift", 0))
        bt_ld = case.N + o.get("bt_ld_extra", 0)
        bt = Buf(torch.full((case.K, case.N), FILL_BF16), case.N + 8, FILL_BF16, torch.bfloat16, o.get("bt_shift", 0))
        with pytest.raises(RuntimeError):
            nat.gemm_bf16_bt(A.ptr, B.ptr, C.ptr, bias.ptr, M, N, K, case.K + G.PAD, case.K + G.PAD, case.N,
                             o.get("epi", G.EPI_BIAS_RELU), f32, aux.ptr, bt.ptr, bt_ld, _st())
        torch.cuda.synchronize()
        assert C.untouched() and aux.untouched() and bt.untouched(), what
        print("  refused: " + what)


def test_ex_colsum_refused_on_the_generic_path():
    """colsum with trans_a = 0 on a shape the LDS-DMA kernels do not take: hipErrorNotSupported before anything is
    launched - C and colsum keep their fill."""
    nat = _nat()
    for name, what in G.EX_REJECTED:
        case = G.CASE[name]
        p = G.problem(name, "unit")
        A, B, lda, ldb = _operands(case, p)
        C = Buf(torch.full((case.M, case.N), FILL_BF16), case.N, FILL_BF16, torch.bfloat16)
        cs = Buf(torch.full((1, case.M), FILL_F32), case.M, FILL_F32, torch.float32)
        with pytest.raises(RuntimeError):
            nat.gemm_bf16_ex(A.ptr, B.ptr, C.ptr, 0, case.M, case.N, case.K, lda, ldb, case.N, case.ta, case.tb,
                             G.EPI_NONE, 0, 0, 0, cs.ptr, _st())
        torch.cuda.synchronize()
        assert C.untouched() and cs.untouched(), what
        print("  refused: %s %s" % (name, what))


def test_null_aux_is_refused_by_the_epilogues_that_read_it():
    """EPI_RELU_MASK / EPI_GELU_GRAD with aux = null, on an LDS-DMA shape and a generic one: an error, C untouched."""
    nat = _nat()
    for name in ("bm64_nn_1", "gen_k600_nn"):
        case = G.CASE[name]
        p = G.problem(name, "unit")
        A, B, lda, ldb = _operands(case, p)
        C = Buf(torch.full((case.M, case.N), FILL_BF16), case.N, FILL_BF16, torch.bfloat16)
        cs = Buf(torch.full((1, case.M), FILL_F32), case.M, FILL_F32, torch.float32)
        for epi in (G.EPI_RELU_MASK, G.EPI_GELU_GRAD):
            with pytest.raises(RuntimeError):
                nat.gemm_bf16(A.ptr, B.ptr, C.ptr, 0, case.M, case.N, case.K, lda, ldb, case.N, case.ta, case.tb, epi, 0, 0,
                              0, _st())
            with pytest.raises(RuntimeError):
                nat.gemm_bf16_ex(A.ptr, B.ptr, C.ptr, 0, case.M, case.N, case.K, lda, ldb, case.N, case.ta, case.tb, epi, 0,
                                 0, 0, cs.ptr, _st())
        torch.cuda.synchronize()
        assert C.untouched() and cs.untouched(), name


def test_no_case_skips_on_256_cus():
    cus = _cus()
    print("device: %d CUs" % cus)
    if cus != 256:
        pytest.skip("a %d-CU device: the case table is sized for 256" % cus)
    for case in G.CASES:
        for v in case.variants:
            assert G.kernel_of(case, v, cus)[0] == case.kernel, (case.name, v.name)


# ------------------------------------------------------------------------------------------------ dct_bias_act_bwd
@pytest.mark.parametrize("act", [G.ACT_NONE, G.ACT_RELU, G.ACT_GELU])
def test_bias_act_bwd(act):
    """Every shape of the table, dZ set and null, accumulate_bias 1 and 0 onto a dbias holding values, and flag 0 onto
    NaN: dbias = the sum whatever it held."""
    nat = _nat()
    nan = float("nan")
    for M, N, pad, shift in G.BAB_SHAPES:
        p = G.bab_problem(M, N, act)
        ld = N + pad
        kernel = G.bab_kernel(M, N, ld, shift)
        dy = Buf(p["dy"], ld, nan, torch.bfloat16, shift)
        aux = Buf(p["aux"], ld, nan, torch.bfloat16, shift)
        for flag, prefill, with_dz in ((1, "values", True), (0, "values", True), (0, "nan", True), (0, "values", False),
                                      (1, "values", False)):
            what = "M=%d N=%d ld=%d shift=%d act=%d flag=%d dbias0=%s dZ=%s [%s, %d row blocks]" % (
                M, N, ld, shift, act, flag, prefill, with_dz, kernel, G.bab_row_blocks(M, N))
            dz = Buf(torch.full((M, N), FILL_BF16), ld, FILL_BF16, torch.bfloat16, shift)
            db0 = p["db0"] if prefill == "values" else torch.full((N,), nan)
            db = Buf(db0.reshape(1, N), N, FILL_F32, torch.float32)
            nat.bias_act_bwd(dy.ptr, aux.ptr if act else 0, dz.ptr if with_dz else 0, db.ptr, M, N, ld, act, flag, _st())
            torch.cuda.synchronize()
            want = G.bab_expect(p, act, flag)
            rs = [_ratio("dct_bias_act_bwd", what, "dbias", db.data().reshape(N), *want["dbias"])]
            if with_dz:
                rs.append(_ratio("dct_bias_act_bwd", what, "dZ", dz.data(), *want["dZ"]))
                assert dz.guards_intact(), what + ": wrote outside dZ"
            else:
                assert dz.untouched(), what + ": dZ written though null was passed"
            assert db.guards_intact() and dy.untouched() and aux.untouched(), what
            assert max(rs) <= 1.0, (what, rs)


def test_bias_act_bwd_refuses_a_null_aux():
    nat = _nat()
    p = G.bab_problem(65, 136, G.ACT_RELU)
    dy = Buf(p["dy"], 136, float("nan"), torch.bfloat16)
    dz = Buf(torch.full((65, 136), FILL_BF16), 136, FILL_BF16, torch.bfloat16)
    db = Buf(p["db0"].reshape(1, 136), 136, FILL_F32, torch.float32)
    for act in (G.ACT_RELU, G.ACT_GELU):
        with pytest.raises(RuntimeError):
            nat.bias_act_bwd(dy.ptr, 0, dz.ptr, db.ptr, 65, 136, 136, act, 0, _st())
    torch.cuda.synchronize()
    assert dz.untouched() and db.untouched()


def test_zz_report_worst_ratios():
    """The worst error / bound per launcher and tensor over this module's run (the figures of the docstring)."""
    for (launcher, tensor), r in sorted(WORST.items()):
        print("WORST %-40s %-8s %.4f" % (launcher, tensor, r))
    assert all(r <= 1.0 for r in WORST.values())
