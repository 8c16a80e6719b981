"""tests/attn_ln_cases.py against itself, without a GPU.

(1) The case tables reach every kernel and instantiation of csrc/attention.hip and of the LayerNorm and gather part of
csrc/nn_kernels.hip, the second grid-stride passes, the shared slot rows and every refusal.  (2) Torch fp32 / bf16
emulations of the kernels, with .to(bfloat16) at exactly their rounding sites (the hidden ones of the MFMA path
included), stay inside the derived bounds on both input sets for every case the GPU test runs, and the inputs keep the
references' own conditions: a GPU failure is then the kernel's, not the bound's.  (3) Mutated emulations - a dropped
key, swapped heads, a forgotten scale, delta, eps, dres or slot row ... - each exceed 1 on the tensor they damage, on at
least one case the GPU test runs: a bound that let one through would be too loose."""
import functools

import pytest
import torch

import attn_ln_cases as C


def _show(what, ratios):
    print("  %s: %s" % (what, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    return ratios


# ------------------------------------------------------------------------------------------------ tables
def test_attention_tables_reach_every_kernel_and_refusal():
    fwd = {C.attn_kernel(c, False) for c in C.ATT_CASES}
    bwd = {C.attn_kernel(c, True) for c in C.ATT_CASES if not c["fwd_only"]}
    for tt in (1, 2, 3, 4):
        for dt in (1, 2, 4):
            assert "attn_fwd_mfma<%d, %d>" % (tt, dt) in fwd and "attn_bwd_mfma<%d, %d>" % (tt, dt) in bwd
    assert "attn_fwd_kernel" in fwd and "attn_bwd_kernel" in bwd and "refused" not in fwd | bwd
    for c in C.ATT_MFMA:  # each of the twelve with one wave live, six waves (a dead half block) and five
        assert C.is_mfma(C.attn_kernel(c, False)) and C.is_mfma(C.attn_kernel(c, True))
    assert {(c["Bsz"], c["H"]) for c in C.ATT_MFMA} == {(1, 1), (2, 3), (5, 1)}
    assert any(c["pad_q"] and c["pad_o"] for c in C.ATT_MFMA)
    sc = [c for c in C.ATT_SCALAR]
    assert all(C.attn_kernel(c, False) == "attn_fwd_kernel" for c in sc)
    assert {c["T"] for c in sc} >= {1, 6, 15, 17, 33, 80, 256, 257, 512}
    assert {c["D"] for c in sc if c["T"] == 17} >= {1, 5, 16, 40, 63, 64}
    assert any(c["T"] == 512 and c["D"] == 16 and not c["fwd_only"] for c in sc)
    assert any(c["T"] == 512 and c["D"] == 64 and c["fwd_only"] for c in sc)
    assert any(C.att_ld(c)[0] != 3 * c["H"] * c["D"] for c in sc)
    # the fallbacks are MFMA-shaped and take the scalar backward; only a misaligned o or do leaves the forward on MFMA
    for c in C.ATT_FALLBACK:
        assert (c["T"], c["D"]) == (32, 32) and C.attn_kernel(c, True) == "attn_bwd_kernel", c
        assert C.is_mfma(C.attn_kernel(c, False)) == bool(set(c["shift"]) & {"o", "do"}), c
    assert any(c["shift"].get("qkv", 0) * 2 % 8 for c in C.ATT_FALLBACK)
    assert any(C.att_ld(c)[0] % 4 for c in C.ATT_FALLBACK)
    for name, c in C.ATT_REFUSED.items():
        assert C.attn_kernel(c, False) == C.attn_kernel(c, True) == "refused", name
    for name, c in C.ATT_REFUSED_BWD_ONLY.items():
        assert C.attn_kernel(c, False) == "attn_fwd_kernel" and C.attn_kernel(c, True) == "refused", name


def test_layernorm_tables_reach_every_kernel_pass_and_refusal():
    lprs = (1, 2, 4, 8, 16, 32, 64)
    fwd = {C.ln_fwd_kernel(M, N) for N in C.LN_FWD_NS for M in C.LN_MS}
    assert fwd == {"layernorm_fwd_kernel"} | {"layernorm_fwd_small<%d>" % l for l in lprs}
    assert C.ln_fwd_kernel(1, 2049) == "refused" and C.ln_fwd_kernel(1, 2048) != "refused"
    assert C.ln_fwd_kernel(37, 64, aligned=False) == "layernorm_fwd_kernel"        # b (or w) one float into a buffer
    assert C.ln_fwd_kernel(*C.LN_FWD_BIG) == "layernorm_fwd_small<64>" and C.ln_fwd_passes(*C.LN_FWD_BIG) == 2
    assert all(C.ln_fwd_passes(M, N) == 1 for N in C.LN_FWD_NS for M in C.LN_MS)
    # lane groups with idle lanes, the single lane, the widest
    assert {N for N in C.LN_FWD_NS if C.ln_lpr(N) and 4 * C.ln_lpr(N) != N} >= {12, 20, 48, 68, 132, 252}
    assert {N for N in C.LN_BWD_EX_NS if 4 * C.ln_lpr(N) != N} >= {12, 20, 48, 68, 132, 252}
    ex = {C.ln_bwd_kernel(M, N, True) for N in C.LN_BWD_EX_NS for M in C.LN_MS}
    assert ex == {"layernorm_bwd_small<%d>" % l for l in lprs}
    (m1, n1), (m2, n2) = C.LN_BWD_EX_BIG
    assert 16 < C.ln_bwd_grid(m1, n1, True)[1] < 32                                  # some slot rows shared, some not
    assert int(C.ln_bwd_row_block(m1, n1).max()) + 1 == C.ln_bwd_grid(m1, n1, True)[1]
    rpb, grid = C.ln_bwd_grid(m2, n2, True)
    assert grid == 1024 and m2 > rpb * grid                                          # a second grid-stride pass
    for M, N in C.LN_BWD_BIG:
        rpb, grid = C.ln_bwd_grid(M, N, False)
        assert grid == 1024 and M > rpb * grid
    assert {C.ln_bwd_kernel(M, N, False) for N in C.LN_BWD_NS for M in C.LN_MS} == {"layernorm_bwd_kernel"}
    assert C.ln_bwd_kernel(1, 2049, False) == "refused"
    for name, r in C.LN_BWD_EX_REFUSED.items():
        aligned = r.get("shift") not in ("w",)
        # dres / dx2 are checked by the launcher next to ln_lpr: every entry names one violated precondition
        bad = [r["N"] % 4 != 0, r["N"] > 256 and r.get("shift") is None, not r.get("ws", True), "shift" in r]
        assert sum(bad) == 1, name
        if r.get("shift") in (None, "w"):
            assert C.ln_bwd_kernel(5, r["N"], True, aligned=aligned, ws=r.get("ws", True)) == "refused", name
    assert len(set(C.LN_BWD_EX_MODES)) == len(C.LN_BWD_EX_MODES) == 32               # every combination, once
    assert C.LN_BWD_EX_MODES[:3] == C.LN_BWD_EX_USED
    assert set(C.LN_BWD_EX_GRADS) == {"wb", "w", "b", ""}
    assert [C.ln_bwd_fold_runs(g) for g in ("wb", "w", "b", "")] == [True, True, True, False]


def test_gather_tables_reach_both_kernels_a_second_pass_and_the_refusal():
    k = {n: C.gather_kernel(c) for n, c in C.GATHER_CASES.items()}
    assert set(k.values()) == {"gather_rows16_kernel", "gather_rows4_kernel"}
    assert k["20-byte rows"] == k["48-byte rows, source 4 bytes off"] == "gather_rows4_kernel"
    assert k["48-byte rows"] == k["1024-byte rows"] == "gather_rows16_kernel"
    for kern in set(k.values()):
        assert {C.gather_passes(c) for n, c in C.GATHER_CASES.items() if k[n] == kern} == {1, 2}, kern
    c = C.GATHER_CASES["second grid-stride pass"]
    assert (c["n_rows"], c["row_bytes"]) == (8200, 1024) and c["n_rows"] * 64 == 524800 > C.GATHER_GRID_VECTORS
    assert [C.gather_kernel(c) for c in C.GATHER_REFUSED.values()] == ["refused"]
    assert [C.gather_kernel(c) for c in C.GATHER_EMPTY.values()] == ["nothing"]
    for name, c in C.GATHER_CASES.items():
        src, idx = C.gather_inputs(c)
        assert idx.dtype == torch.int32 and idx.numel() == c["n_rows"] and 0 <= int(idx.min())
        assert int(idx.max()) < c["src_rows"], name
        if c["n_rows"] >= 2 and c["idx"] != "repeated":
            assert {0, c["src_rows"] - 1} <= set(idx.tolist()), name
        assert C.gather_ref(src, idx).shape == (c["n_rows"], c["row_bytes"])
    rep = C.gather_inputs(C.GATHER_CASES["repeated indices"])[1]
    assert len(set(rep.tolist())) < rep.numel()


# ------------------------------------------------------------------------------------------------ attention
@functools.lru_cache(maxsize=None)
def _att_fwd(i, kind):
    """(inputs, scale, emulated forward of the path the launcher takes) of ATT_CASES[i]; nothing changes it."""
    c = C.ATT_CASES[i]
    q, k, v, do = C.att_inputs(c, kind)
    scale = C.f32scale(c["D"])
    return (q, k, v, do), scale, C.emulate_attn_fwd(q, k, v, scale, C.is_mfma(C.attn_kernel(c, False)))


ATT_IDS = [C.att_name(c) for c in C.ATT_CASES]


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("i", range(len(C.ATT_CASES)), ids=ATT_IDS)
def test_attention_emulation_inside_the_bounds(i, kind):
    c = C.ATT_CASES[i]
    (q, k, v, do), scale, g = _att_fwd(i, kind)
    r = C.attn_fwd_check(g, q, k, v, scale, C.is_mfma(C.attn_kernel(c, False)))
    if not c["fwd_only"]:
        mf = C.is_mfma(C.attn_kernel(c, True))
        gb = C.emulate_attn_bwd(q, k, v, g["o"], g["lse"], do, scale, mf)
        r.update(C.attn_bwd_check(gb, q, k, v, g["o"], g["lse"], do, scale, mf))
    _show("%s %s" % (C.att_name(c), kind), r)
    assert max(r.values()) <= 1.0, r


def test_attention_edge_set_reaches_what_it_is_meant_to():
    big_lse, flushed = 0.0, False
    for i, c in enumerate(C.ATT_CASES):
        (q, k, v, do), scale, g = _att_fwd(i, "edge")
        big_lse = max(big_lse, float(g["lse"].abs().max()))
        y = (q.double() @ k.double().transpose(-1, -2)) * scale
        flushed = flushed or bool(((y - y.max(-1, keepdim=True).values) < -88.0).any())
        assert 1e-4 <= float(do.float().abs().max()) <= 8.0
    assert big_lse > 30.0 and flushed


def _mutant_worst(mutants, run):
    worst = {m: 0.0 for m in mutants}
    for m in mutants:
        for kind in C.INPUT_SETS:
            for i, c in enumerate(C.ATT_CASES):
                if c["T"] > 64 or c["H"] < 2:  # the small cases suffice; heads_swapped needs two heads
                    continue
                worst[m] = max(worst[m], run(m, i, c, kind))
    return worst


def test_attention_forward_mutants_outside_the_bounds():
    def run(m, i, c, kind):
        (q, k, v, do), scale, _ = _att_fwd(i, kind)
        mf = C.is_mfma(C.attn_kernel(c, False))
        return C.attn_fwd_check(C.emulate_attn_fwd(q, k, v, scale, mf, mutant=m), q, k, v, scale, mf)[
            C.ATT_FWD_MUTANTS[m]]
    worst = _show("forward mutants", _mutant_worst(C.ATT_FWD_MUTANTS, run))
    assert min(worst.values()) > 1.0, worst


def test_attention_backward_mutants_outside_the_bounds():
    def run(m, i, c, kind):
        (q, k, v, do), scale, g = _att_fwd(i, kind)
        mf = C.is_mfma(C.attn_kernel(c, True))
        gb = C.emulate_attn_bwd(q, k, v, g["o"], g["lse"], do, scale, mf, mutant=m)
        return C.attn_bwd_check(gb, q, k, v, g["o"], g["lse"], do, scale, mf)[C.ATT_BWD_MUTANTS[m]]
    worst = _show("backward mutants", _mutant_worst(C.ATT_BWD_MUTANTS, run))
    assert min(worst.values()) > 1.0, worst


def test_fallback_cases_would_show_the_mfma_kernel():
    """What the fallback cases are held to is the scalar path's bound, and it is the tighter one: the MFMA emulation
    (bf16 P and dS) exceeds it on every fallback case, so a fallback that silently took the MFMA kernel would fail."""
    for c in C.ATT_FALLBACK:
        q, k, v, do = C.att_inputs(c, "unit")
        scale = C.f32scale(c["D"])
        g = C.emulate_attn_fwd(q, k, v, scale, True)
        r = C.attn_fwd_check(g, q, k, v, scale, False)
        gb = C.emulate_attn_bwd(q, k, v, g["o"], g["lse"], do, scale, True)
        r.update(C.attn_bwd_check(gb, q, k, v, g["o"], g["lse"], do, scale, False))
        _show("MFMA emulation under the scalar bound, %s" % C.att_name(c), r)
        assert r["o"] > 1.0 and max(r["dq"], r["dk"], r["dv"]) > 1.0, r


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_FWD_GROUPS = [[(M, N) for M in C.LN_MS] for N in C.LN_FWD_NS] + [[C.LN_FWD_BIG]]


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("shapes", LN_FWD_GROUPS, ids=lambda g: "M%d_N%d" % g[-1])
def test_layernorm_forward_emulation_inside_the_bounds_and_the_variance_condition(shapes, kind):
    for M, N in shapes:
        for in_bf16, out_bf16 in C.LN_FWD_DTYPES if M < 1000 else ((0, 0), (1, 1)):
            i = C.ln_inputs(M, N, kind, in_bf16)
            for nulls in ("",) + (C.LN_FWD_NULLS if (M, N) in ((37, 64), (37, 260)) else ()):
                w, b = (None if "w" in nulls else i["w"]), (None if "b" in nulls else i["b"])
                g = C.emulate_ln_fwd(i["x"], w, b, out_bf16)
                r = C.ln_fwd_check(g, i["x"], w, b, out_bf16)
                assert max(r.values()) <= 1.0, (M, N, in_bf16, out_bf16, nulls, r)
            _show("M=%d N=%d %s in_bf16=%d out_bf16=%d" % (M, N, kind, in_bf16, out_bf16), r)
            # the references' own condition: every row but the ill-conditioned one the edge set carries on purpose
            cond = C.ln_ref(i["x"].double(), i["w"], i["b"], out_bf16)["cond"]
            bad = set(torch.nonzero(~cond)[:, 0].tolist())
            assert bad <= ({C.BIG_ROW} if kind == "edge" else set()), (M, N, in_bf16, bad)
    if kind == "edge" and shapes[-1] == (37, 64):  # and that row does break it in fp32: it is what it is meant to be
        i = C.ln_inputs(37, 64, "edge", 0)
        assert not bool(C.ln_ref(i["x"].double(), i["w"], i["b"], 0)["cond"][C.BIG_ROW])
        assert bool((i["x"][C.CONST_ROW] == C.CONST_VAL).all())


def test_layernorm_forward_mutants_outside_the_bounds():
    worst = {m: 0.0 for m in C.LN_FWD_MUTANTS}
    for m, hit in C.LN_FWD_MUTANTS.items():
        for kind in C.INPUT_SETS:
            for M, N in ((5, 12), (37, 64), (37, 260)):
                i = C.ln_inputs(M, N, kind, 0)
                g = C.emulate_ln_fwd(i["x"], i["w"], i["b"], 0, mutant=m)
                worst[m] = max(worst[m], C.ln_fwd_check(g, i["x"], i["w"], i["b"], 0)[hit])
    _show("forward mutants", worst)
    assert min(worst.values()) > 1.0, worst
    i = C.ln_inputs(37, 64, "edge", 0)  # eps omitted: the constant row
    g = C.emulate_ln_fwd(i["x"], i["w"], i["b"], 0, mutant="eps_omitted")
    ref = C.ln_ref(i["x"].double(), i["w"], i["b"], 0)
    err = (g["rstd"].double() - ref["rstd"]).abs()
    assert not bool(err[C.CONST_ROW] <= ref["e_rstd"][C.CONST_ROW])


def _ln_saved(i):
    """mean / rstd as a forward launch saves them (fp32)."""
    g = C.emulate_ln_fwd(i["x"], i["w"], i["b"], 0)
    return g["mean"], g["rstd"]


def _ln_bwd_run(M, N, kind, ex, mode, mutant=None):
    dy_bf16, x_bf16, dx_bf16, dx2, dres = mode
    i = C.ln_inputs(M, N, kind, x_bf16, dy_bf16)
    mean, rstd = _ln_saved(i)
    dr = i["dres"] if dres else None
    g = C.emulate_ln_bwd(i["dy"], i["x"], i["w"], mean, rstd, dr, i["dw0"], i["db0"], dx_bf16, mutant=mutant,
                         row_block=C.ln_bwd_row_block(M, N) if ex else None)
    return C.ln_bwd_check(g, i["dy"], i["x"], i["w"], mean, rstd, dr, i["dw0"], i["db0"], C.ln_bwd_adders(M, N, ex),
                          dx_bf16)


@pytest.mark.parametrize("kind", C.INPUT_SETS)
def test_layernorm_backward_emulation_inside_the_bounds(kind):
    for M, N in [(M, N) for N in C.LN_BWD_EX_NS for M in C.LN_MS] + list(C.LN_BWD_EX_BIG):
        for mode in C.LN_BWD_EX_MODES if M < 1000 else C.LN_BWD_EX_MODES[:1]:
            r = _ln_bwd_run(M, N, kind, True, mode)
            assert set(r) == {"dx", "dw", "db"} and max(r.values()) <= 1.0, (M, N, mode, r)
        _show("bwd_ex M=%d N=%d %s" % (M, N, kind), r)
    for M, N in [(M, N) for N in C.LN_BWD_NS for M in C.LN_MS] + list(C.LN_BWD_BIG):
        for io in (0, 1):
            r = _ln_bwd_run(M, N, kind, False, (io, io, io, 0, 0))
            assert max(r.values()) <= 1.0, (M, N, io, r)
        _show("bwd M=%d N=%d %s" % (M, N, kind), r)


def test_layernorm_backward_mutants_outside_the_bounds():
    worst = {m: 0.0 for m in C.LN_BWD_MUTANTS}
    for m, hit in C.LN_BWD_MUTANTS.items():
        for kind in C.INPUT_SETS:
            for M, N in ((37, 12), (300, 64)):
                worst[m] = max(worst[m], _ln_bwd_run(M, N, kind, True, (1, 0, 0, 1, 1), mutant=m)[hit])
    _show("backward mutants", worst)
    assert min(worst.values()) > 1.0, worst
