"""tests/skinny_cases.py against itself, on the CPU: a torch fp32 / bf16 emulation of the skinny, fused-head and loss
kernels sits inside every bound, every named mutant falls outside somewhere, and the tables reach every template
instantiation and path the launchers hold."""
import pytest
import torch

import skinny_cases as S

KINDS = (0, 1)  # CE, MSE


def _r(got, ref):
    return {k: S.ratio(got[k], *ref[k]) for k in ref if got.get(k) is not None}


# ------------------------------------------------------------------------------------------------ skinny fwd / dx / dw
@pytest.mark.parametrize("B,K,C", S.sk_cases() + [S.SK_DX_GRID_STRIDE])
def test_skinny_emulation_is_inside_every_bound(B, K, C):
    p = S.sk_problem(B, K, C)
    for with_bias in (True, False):
        r = S.ratio(S.sk_emulate(p, "fwd", with_bias=with_bias), *S.sk_fwd_expect(p, with_bias))
        assert r <= 1.0, ("fwd", with_bias, r)
    for masked in (True, False):
        r = S.ratio(S.sk_emulate(p, "dx", masked=masked), *S.sk_dx_expect(p, masked))
        assert r <= 1.0, ("dx", masked, r)
    r = _r(S.sk_emulate(p, "dw"), S.sk_dw_expect(p))
    print("  skinny %s: dw %s" % ((B, K, C), r))
    assert all(x <= 1.0 for x in r.values()), r


def test_skinny_mutants_are_outside():
    p = S.sk_problem(65, 1024, 3)
    m = "last_class_weights_for_c_minus_2"
    assert S.ratio(S.sk_emulate(p, "fwd", m), *S.sk_fwd_expect(p)) > 1.0
    assert S.ratio(S.sk_emulate(p, "dx", m), *S.sk_dx_expect(p, True)) > 1.0
    for B, K, C in [(65, 1024, 3), (777, 1024, 2), (3, 520, 5)]:
        p = S.sk_problem(B, K, C)
        assert S.dw_geometry(B, K)[0] == 2
        r = _r(S.sk_emulate(p, "dw", "db_once_per_column_block"), S.sk_dw_expect(p))
        assert r["db"] > 1.0 and r["dW"] <= 1.0, r


def test_skinny_table_covers_the_templates_and_the_tails():
    cases = S.sk_cases()
    assert {S.ct_of(C) for _, _, C in cases} == {1, 2, 4, 8}
    assert {C for _, _, C in cases if C != S.ct_of(C)} == {3, 5}  # class slots past C: the re-read of row C - 1
    for C in S.SK_CS:
        assert {K for _, K, c in cases if c == C} == set(S.SK_KS)
    assert {B for B, _, _ in cases} == set(S.SK_BS)
    assert all(K % 8 == 0 for K in S.SK_KS) and any(K % 512 for K in S.SK_KS) and 8 in S.SK_KS
    # K = 8, 264, 520: lanes of skinny_dw's last column block past K (kc = 0)
    assert all(K % 512 for K in (8, 264, 520))
    geo = {(B, K): S.dw_geometry(B, K) for B, K, _ in cases}
    assert any(ny == 1 for _, ny, _ in geo.values()) and any(ny > 1 for _, ny, _ in geo.values())
    assert any(ny > 1 and rp % 32 for _, ny, rp in geo.values())
    B, K, _ = S.SK_DX_GRID_STRIDE
    assert B * K // 8 > 4096 * 256


# ------------------------------------------------------------------------------------------------ fused head
@pytest.mark.parametrize("case", S.head_cases(), ids=lambda c: "B%d_K%d_C%d" % c[:3])
def test_head_emulation_is_inside_every_bound(case):
    B, K, C, mask, nulls, gs, ls = case
    p = S.head_problem(B, K, C)
    for kind in KINDS:
        r = S.head_check(S.head_emulate(p, kind, mask, gs, ls, "bias" not in nulls), p, kind, mask, gs, ls,
                         "bias" not in nulls)
        print("  head %s kind %d: %s" % (case[:3], kind, ", ".join("%s %.3f" % kv for kv in r.items())))
        assert all(x <= 1.0 for x in r.values()), r


@pytest.mark.parametrize("mutant", S.HEAD_MUTANTS)
def test_head_mutants_are_outside(mutant):
    worst = {}
    for B, K, C, mask, nulls, gs, ls in S.head_cases():
        if nulls or (mutant.startswith("last_class") and C < 2):
            continue
        p = S.head_problem(B, K, C)
        for kind in KINDS:
            r = S.head_check(S.head_emulate(p, kind, mask, gs, ls, mutant=mutant), p, kind, mask, gs, ls)
            for k, x in r.items():
                worst[k] = max(worst.get(k, 0.0), x)
    print("  %s: %s" % (mutant, worst))
    target = {"last_class_weights_for_c_minus_2": "dW", "dz_not_rounded": "dz_is_bf16", "mse_no_1_over_c": "db",
              "ce_no_grad_scale": "dH", "loss_scale_ignored": "loss"}[mutant]
    assert worst[target] > 1.0, (mutant, worst)


def test_head_table_reaches_every_instantiation():
    reached = {S.head_kernel(B, K, C) for B, K, C, *_ in S.head_cases()}
    assert reached == set(S.HEAD_INSTANCES), set(S.HEAD_INSTANCES) ^ reached
    assert len(S.HEAD_INSTANCES) == 15
    cases = S.head_cases()
    assert {B for B, *_ in cases} >= {1, 5, 17, 130, 4099}
    assert {m for _, _, _, m, *_ in cases} == {0, 1}
    seen = {n for c in cases for n in c[4]}
    assert seen == {"dH", "db", "loss_sum", "bias"}
    for B, K, C, *_ in cases:
        assert S.head_supported(K, C)
        y = S.head_problem(B, K, C)["y"]
        assert int(y[0]) == C - 1 and (B < C or set(y.tolist()) == set(range(C)))
    assert 4099 % 32  # a ragged last block of 8 waves x 4 rows


def test_head_supported_rule():
    want = {(512, 1): 1, (2048, 2): 1, (2560, 2): 0, (1536, 3): 0, (1024, 4): 1, (1024, 5): 0, (512, 8): 1, (512, 9): 0,
            (520, 2): 0, (256, 1): 0, (0, 1): 0, (512, 0): 0, (1024, 8): 0}
    assert set(S.HEAD_SUPPORT) == set(want)
    for (K, C), ok in want.items():
        assert S.head_supported(K, C) == bool(ok), (K, C)


# ------------------------------------------------------------------------------------------------ loss kernel
@pytest.mark.parametrize("lbf16", [0, 1])
@pytest.mark.parametrize("C", S.LOSS_CS)
def test_loss_emulation_is_inside_every_bound(C, lbf16):
    for M in S.LOSS_MS:
        p = S.loss_problem(M, C, lbf16)
        for kind in KINDS:
            for gs, ls in ((1.0 / M, 1.0), (1.0 / 3.0, 1.0 / 3.0)):
                r = _r(S.loss_emulate(p, kind, gs, ls, lbf16), S.loss_expect(p, kind, gs, ls, lbf16))
                print("  loss M=%d C=%d bf16=%d kind %d: %s" % (M, C, lbf16, kind, r))
                assert all(x <= 1.0 for x in r.values()), r


@pytest.mark.parametrize("mutant", S.LOSS_MUTANTS)
def test_loss_mutants_are_outside(mutant):
    worst = {}
    for C in (2, 9):
        p = S.loss_problem(1000, C, 0)
        for kind in KINDS:
            r = _r(S.loss_emulate(p, kind, 1.0 / 3.0, 1.0 / 3.0, 0, mutant), S.loss_expect(p, kind, 1.0 / 3.0, 1.0 / 3.0, 0))
            for k, x in r.items():
                worst[k] = max(worst.get(k, 0.0), x)
    target = {"mse_no_1_over_c": "dlogits", "ce_no_grad_scale": "dlogits", "loss_scale_ignored": "loss",
              "ties_take_last": "correct"}[mutant]
    assert worst[target] > 1.0, (mutant, worst)


def test_loss_table_covers_both_paths_ties_and_the_grid_stride():
    assert {S.loss_path(C) for C in S.LOSS_CS} == {"registers (C <= 8)", "generic loop (C > 8)"}
    assert {S.loss_path(C) for C, _, _ in S.LOSS_BIG} == {"registers (C <= 8)", "generic loop (C > 8)"}
    assert S.loss_geometry(S.LOSS_BIG_M) == (1024, 2) and S.loss_geometry(1000) == (4, 1)
    for C in (2, 9):
        z = S.loss_problem(1000, C, 0)["z"]
        m = z.max(-1, keepdim=True).values
        ties = ((z == m).sum(-1) > 1)
        assert int(ties.sum()) >= 200
        # a tie whose first and last holder differ, with the label on one of them: ties_take_last changes the count
        assert float(z.abs().max()) <= 30.0 and float(z.abs().max()) > 20.0
