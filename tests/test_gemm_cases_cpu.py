"""tests/gemm_cases.py against itself, on the CPU: a torch fp32 / bf16 emulation of every launch sits inside every bound,
every named mutant falls outside on the case meant to catch it, the dispatch mirror reaches every kernel name in every
transpose at 256 CUs, and the tables hold the conditions the launchers state."""
import pytest
import torch

import gemm_cases as G

CUS = 256


def _kinds(name):
    return ("unit",) if name in G.BIG else G.INPUT_SETS


def _ratios(case, v, kind, mutant=None):
    p = G.problem(case.name, kind)
    _, splits, adds = G.launch_plan(case, v, CUS)
    want = G.expect(p, v, splits, colsum_adds=adds)
    got = G.emulate(p, v, splits, mutant)
    return {k: G.ratio(got[k], *want[k]) for k in want}


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_emulation_is_inside_every_bound(name):
    case = G.CASE[name]
    for kind in _kinds(name):
        for v in case.variants:
            r = _ratios(case, v, kind)
            print("  %s %s %s: %s" % (name, kind, v.name, ", ".join("%s %.3f" % kv for kv in r.items())))
            assert all(x <= 1.0 for x in r.values()), (name, kind, v.name, r)


@pytest.mark.parametrize("mutant", list(G.GEMM_MUTANTS))
def test_every_mutant_is_outside_its_bound(mutant):
    tensor = G.GEMM_MUTANTS[mutant]
    for name, vname in G.MUTANT_CASES[mutant]:
        case = G.CASE[name]
        v = next(x for x in case.variants if x.name == vname)
        worst = max(_ratios(case, v, kind, mutant)[tensor] for kind in _kinds(name))
        print("  %s on %s %s: %s error / bound %.3g" % (mutant, name, vname, tensor, worst))
        assert worst > 1.0, (mutant, name, vname, worst)


def test_every_listed_mutant_has_a_case():
    assert set(G.MUTANT_CASES) == set(G.GEMM_MUTANTS)


def test_case_table_reaches_every_kernel_at_256_cus():
    reached = {}
    for case in G.CASES:
        for v in case.variants:
            k, splits = G.kernel_of(case, v, CUS)
            assert k == case.kernel, (case.name, v.name, k, case.kernel)
            reached.setdefault(k, []).append(case.name)
            if "split" in k:
                assert splits > 1 and len(G.slices(case.K, splits)) == splits
    assert set(reached) == set(G.ALL_KERNELS), set(G.ALL_KERNELS) ^ set(reached)
    # the entry points over the kernels the issue names for them
    bt = {c.kernel for c in G.CASES if any(v.entry == "bt" for v in c.variants)}
    assert bt == {"bm64<1>", "k128<0,1>", "tile128<0,1>"}
    for k in bt:  # each with a ragged last column tile (N % 8 == 0) and both bt_ld = N and N + 8
        cs = [c for c in G.CASES if c.kernel == k and c.variants[0].entry == "bt"]
        assert any(c.N % 128 and c.N % 8 == 0 for c in cs), k
        assert {bool(v.ldc_pad) for c in cs if c.N % 128 for v in c.variants} == {False, True}, k
    # the 8-wave kernel with two 128-deep stages and with three (a refilled buffer), in every transpose
    for ta in (0, 1):
        for tb in (0, 1):
            assert {c.K for c in G.CASES if c.kernel == "k128<%d,%d>" % (ta, tb)} >= {256, 384}, (ta, tb)
    res = {c.kernel.split("<")[0] for c in G.CASES if any(v.entry == "residual" for v in c.variants)}
    assert res == {"bm64", "generic"}
    # both forms of the reduce pass, uneven slices, a refilled LDS buffer
    two_pass = [c for c in G.CASES if c.kernel.startswith("split2pass")]
    assert {G.reduce_variant(c.N) for c in two_pass} == {"float4", "scalar"}
    assert any(len({b - a for a, b in G.slices(c.K, G.kernel_of(c, c.variants[0], CUS)[1])}) == 2 for c in two_pass)
    assert any(c.K // 64 >= 5 for c in G.CASES if c.kernel.startswith("bm64"))


def test_variants_cover_epilogues_outputs_and_strides():
    seen = {(v.epi, v.out_f32) for c in G.CASES for v in c.variants if v.entry in ("gemm", "ex")}
    for epi in range(6):
        assert (epi, 0) in seen, epi
    for epi in (G.EPI_NONE, G.EPI_BIAS, G.EPI_RELU_MASK, G.EPI_GELU_GRAD):
        assert (epi, 1) in seen, epi
    for k in G.ALL_KERNELS:
        vs = [v for c in G.CASES if c.kernel == k for v in c.variants]
        assert any(v.ldc_pad for v in vs) and any(not v.ldc_pad for v in vs), k
        if not k.startswith("tile128<0"):
            assert any(v.acc for v in vs), k
    assert {c.ld for c in G.CASES} >= {0, G.PAD, "odd", "unaligned"}


def test_generic_cases_name_their_reason():
    """Each generic case fails gemm_v2_ok, and without its stated defect the same shape would pass it."""
    for c in G.CASES:
        if not c.kernel.startswith("generic"):
            continue
        lda, ldb, shift = G.leading(c)
        assert not G.v2_ok(c.M, c.N, c.K, c.ta, c.tb, lda, ldb, shift == 0), c.name
    assert G.v2_ok(136, 72, 64, 1, 0, 136, 72) and not G.v2_ok(133, 72, 64, 1, 0, 136, 72)
    assert G.v2_ok(130, 72, 64, 0, 0, 64, 72) and not G.v2_ok(130, 70, 64, 0, 0, 64, 72)
    assert G.v2_ok(1, 72, 64, 0, 1, 64, 64) and G.v2_ok(130, 3, 64, 0, 1, 64, 64)
    assert not G.v2_ok(130, 72, 64, 0, 1, 64, 64, epi_aligned=False)
    name, v, kernel = G.UNALIGNED_BIAS
    assert G.kernel_of(G.CASE[name], v, CUS, epi_aligned=False)[0] == kernel
    name, v, kernel = G.UNALIGNED_RESIDUAL
    assert v.entry == "residual" and G.kernel_of(G.CASE[name], v, CUS, epi_aligned=False)[0] == kernel
    assert G.kernel_of(G.CASE[name], v, CUS)[0] == G.CASE[name].kernel != kernel


def test_dispatch_mirror_follows_the_cu_count():
    # 4096 x 1024 x 1024 forward: 256 tiles, one per CU of a 256-CU device; half-height tiles on a 1024-CU one, plain tiles on 128
    args = (4096, 1024, 1024, 0, 1, 0, G.EPI_BIAS_RELU, False, 0, 1024, 1024, True)
    assert G.gemm_kernel(*args, 256) == ("k128<0,1>", 1)
    assert G.gemm_kernel(*args, 1024) == ("bm64<1>", 1)
    assert G.gemm_kernel(*args, 128) == ("tile128<0,1>", 1)
    # the dW of that layer: 64 tiles, 64 k-tiles -> 4 slices of 16, two passes; 8 slices on 512 CUs, atomics
    dw = (1024, 1024, 4096, 1, 0, 1, G.EPI_NONE, False, 1, 1024, 1024, True)
    assert G.gemm_kernel(*dw, 256) == ("split2pass<1,0>", 4)
    assert G.gemm_kernel(*dw, 512) == ("splitatomic<1,0>", 8)


def test_atomic_accumulate_precondition():
    """expect()'s bound for the atomic form holds |C0| <= sum|a||b| wherever a partial can be non-zero."""
    for c in G.CASES:
        if c.kernel.startswith("splitatomic"):
            for kind in G.INPUT_SETS:
                p = G.problem(c.name, kind)
                live = p["absprod"] > 0
                assert bool((p["c0"].double().abs()[live] <= p["absprod"][live]).all()), (c.name, kind)
                assert c.K / 5 + 2 * 5 <= c.K


def test_relu_mask_aux_has_the_edge_values():
    p = G.problem("bm64_nn_1", "unit")
    a = p["act"].float()
    zeros = float((a == 0).float().mean())
    assert 0.4 < zeros < 0.7, zeros
    assert bool(torch.signbit(a[a == 0]).any()) and bool((a == G.MIN_BF16).any())


# ------------------------------------------------------------------------------------------------ dct_bias_act_bwd
@pytest.mark.parametrize("act", [G.ACT_NONE, G.ACT_RELU, G.ACT_GELU])
def test_bias_act_bwd_emulation_and_mutant(act):
    for M, N, pad, shift in G.BAB_SHAPES:
        p = G.bab_problem(M, N, act)
        for flag in (0, 1):
            want = G.bab_expect(p, act, flag)
            got = G.bab_emulate(p, act, flag)
            r = {k: G.ratio(got[k], *want[k]) for k in want}
            assert all(x <= 1.0 for x in r.values()), (M, N, act, flag, r)
        bad = G.bab_emulate(p, act, 0, "flag0_adds_to_dbias")
        assert G.ratio(bad["dbias"], *G.bab_expect(p, act, 0)["dbias"]) > 1.0, (M, N)


def test_bias_act_bwd_table_reaches_both_kernels_and_row_blocks():
    kernels = {G.bab_kernel(M, N, N + pad, shift) for M, N, pad, shift in G.BAB_SHAPES}
    assert kernels == {"bias_act_bwd_kernel<true>", "bias_act_bwd_kernel<false>"}
    assert G.bab_row_blocks(64, 136) == 1 and G.bab_row_blocks(65, 136) == 2 and G.bab_row_blocks(333, 1001) == 6
    assert any(shift and N % 8 == 0 for _, N, _, shift in G.BAB_SHAPES)
