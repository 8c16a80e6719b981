"""tests/tt_cases.py against itself, without a GPU.

(1) A torch fp32 emulation of every stage of the TabTransformer block, head and embedding kernels, with .to(bfloat16) at
exactly the kernels' rounding sites (the hidden ones included), stays inside the derived bounds on both input sets and
at every B: a GPU failure is then the kernel's, not the bound's.  (2) Mutated emulations - a dropped key, swapped heads,
a forgotten bias, scale, 1/64 or wrap ... - each exceed 1 on the tensor they damage: a bound that let one through
would be too loose.  (3) Every launch table entry satisfies its launcher's preconditions and every rejected entry
violates exactly one."""
import functools

import pytest
import torch

import tt_cases as C


@functools.lru_cache(maxsize=None)
def _fwd(B, kind, embedded):
    """(params, input, emulated forward) shared by the tests below; nothing changes it."""
    p = C.block_params(kind)
    if embedded:
        emb = C.embed_input(B, kind)
        return p, emb, C.emulate_fwd(p, emb=emb)
    h = C.block_input(B, kind)
    return p, h, C.emulate_fwd(p, h=h)


def _show(what, ratios):
    print("  %s: %s" % (what, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    return ratios


@pytest.mark.parametrize("embedded", [False, True])
@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("B", list(C.BLOCK_BS))
def test_forward_emulation_inside_the_bounds(B, kind, embedded):
    p, x, g = _fwd(B, kind, embedded)
    r = _show("fwd B=%d %s%s" % (B, kind, " embedded" if embedded else ""),
              C.fwd_check(g, p, **({"emb": x} if embedded else {"h": x})))
    assert set(r) == set(C.FWD_OUTPUTS) | {"pool"}
    assert max(r.values()) <= 1.0, r
    if kind == "edge":  # the edge set reaches what it is meant to reach
        assert float(g["rstd1"].max()) > 300.0 and float(g["pre"].float().abs().max()) >= 8.0
        assert float(g["lse"].abs().max()) > 30.0


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("mutant", list(C.FWD_MUTANTS))
def test_forward_mutants_outside_the_bounds(mutant, kind):
    B = 3
    p, h, _ = _fwd(B, kind, False)
    r = C.fwd_check(C.emulate_fwd(p, h=h, mutant=mutant), p, h=h)
    hit = C.FWD_MUTANTS[mutant]
    print("  %s (%s): %s %.2f" % (mutant, kind, hit, r[hit]))
    assert r[hit] > 1.0, (mutant, r)


def _bwd_inputs(B, kind, pooled, embedded):
    p, x, saved = _fwd(B, kind, embedded)
    saved = dict(saved)
    kw = {"init": C.ln_grad_init()}
    if embedded:
        kw["emb"] = x
    else:
        saved["h"] = x
    kw["dpool" if pooled else "dout"] = C.dout_input(B, kind, pooled=pooled)
    return p, saved, kw


@pytest.mark.parametrize("pooled,embedded", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("B", list(C.BLOCK_BS))
def test_backward_emulation_inside_the_bounds(B, kind, pooled, embedded):
    p, saved, kw = _bwd_inputs(B, kind, pooled, embedded)
    g = C.emulate_bwd(p, saved, **kw)
    r = _show("bwd B=%d %s%s%s" % (B, kind, " pooled" if pooled else "", " embedded" if embedded else ""),
              C.bwd_check(g, saved, p, **kw))
    assert set(r) == set(C.BWD_OUTPUTS) | ({"dout16"} if pooled else set())
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("mutant", list(C.BWD_MUTANTS))
def test_backward_mutants_outside_the_bounds(mutant, kind):
    p, saved, kw = _bwd_inputs(3, kind, mutant == "pool_no_64th", False)
    r = C.bwd_check(C.emulate_bwd(p, saved, mutant=mutant, **kw), saved, p, **kw)
    hit = C.BWD_MUTANTS[mutant]
    print("  %s (%s): %s %.2f" % (mutant, kind, hit, r[hit]))
    assert r[hit] > 1.0, (mutant, r)


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("Tn", C.HEAD_TS)
@pytest.mark.parametrize("B", C.HEAD_BS)
def test_head_emulation_inside_the_bounds_and_mutant_outside(B, Tn, kind):
    for Cn in C.HEAD_CS:
        i = C.head_inputs(B, Tn, Cn, kind)
        dl = float(i["dloss"])
        r = _show("head B=%d T=%d C=%d %s" % (B, Tn, Cn, kind),
                  C.head_check(C.emulate_head(i, B, Tn, Cn, dl), i, B, Tn, Cn, dl))
        assert set(r) == {"loss", "dh", "dh16", "dln_w", "dln_b", "dW", "dbias"}
        assert max(r.values()) <= 1.0, (Cn, r)
        if Cn > 1:
            m = C.head_check(C.emulate_head(i, B, Tn, Cn, dl, mutant="dw_last_class_from_0"), i, B, Tn, Cn, dl)
            assert m["dW"] > 1.0, (Cn, m)


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("F", C.EMBED_FS)
@pytest.mark.parametrize("B", C.EMBED_BS)
def test_embedding_references(B, F, kind):
    x, E, c = C.embed_input(B, kind, F=F)
    h, e_h = C.embed_ref(x, E, c)
    assert C.ratio(h.float(), h, e_h) <= 1.0                             # the correctly rounded value
    g = torch.Generator().manual_seed(B + F)
    dh, dE0, dc0 = (torch.randn(*s, generator=g) for s in ((B * F, C.DM), (F, C.DM), (F, C.DM)))
    dE, e_dE, dc, e_dc = C.embed_bwd_ref(x, dh, dE0, dc0)
    d3 = dh.reshape(B, F, C.DM)
    gE, gc = dE0.clone(), dc0.clone()
    for b in range(B):  # fp32, sample by sample
        gE, gc = gE + x[b, :, None] * d3[b], gc + d3[b]
    r = {"dE": C.ratio(gE, dE, e_dE), "dc": C.ratio(gc, dc, e_dc)}
    _show("embed bwd B=%d F=%d %s" % (B, F, kind), r)
    assert max(r.values()) <= 1.0
    assert C.ratio(gE - dE0, dE, e_dE) > 1.0 and C.ratio(gc - dc0, dc, e_dc) > 1.0  # overwritten, not accumulated


@pytest.mark.parametrize("B", list(C.BLOCK_BS))
def test_gather_reference_wraps_and_the_mutant_does_not(B):
    stride, n_items, n_idx, cursors = C.batch_geometry(B)
    X, Y, lists = C.gather_inputs(B)
    for name, idx in lists.items():
        assert idx.numel() == n_idx > n_items and int(idx.max()) < X.shape[0]
        for cursor in cursors:
            rows = C.gather_rows_ref(idx, cursor, stride, n_items, B)
            q = cursor * stride + torch.arange(B)
            assert torch.equal(rows, idx[q % n_items])
            nowrap = C.gather_rows_no_wrap(idx, cursor, stride, n_items, B)  # stays inside the index buffer
            wraps = bool((q >= n_items).any())
            assert wraps == (cursor == 2)
            if wraps and name == "permutation":
                assert not torch.equal(X[rows], X[nowrap])
            if not wraps:
                assert torch.equal(rows, nowrap)


def test_launch_tables_satisfy_the_preconditions_and_rejections_violate_exactly_one():
    for name, m in C.FWD_MODES.items():
        assert C.fwd_violations(**m) == [], name
    for name, rej in C.FWD_REJECTED.items():
        spec = dict(C.FWD_MODES[rej["base"]], **{k: v for k, v in rej.items() if k != "base"})
        assert len(C.fwd_violations(**spec)) == 1, (name, C.fwd_violations(**spec))
    for name, m in C.BWD_MODES.items():
        assert C.bwd_violations(**m) == [], name
    for name, rej in C.BWD_REJECTED.items():
        spec = dict(C.BWD_MODES[rej["base"]], **{k: v for k, v in rej.items() if k != "base"})
        assert len(C.bwd_violations(**spec)) == 1, (name, C.bwd_violations(**spec))
    # the modes models/tabtransformer.py runs, and one of every switch on its own
    for k in ("recomp", "qkv_recomp", "lnrep", "pooled", "embed"):
        assert any(m[k] and sum(bool(m[q]) for q in ("recomp", "qkv_recomp", "lnrep", "pooled", "embed")) == 1
                   for m in C.BWD_MODES.values()), k
    # every launch that recomputes, uses the replicas or stores no dpre has a launch on the same inputs that stores
    # everything to be bit-compared with
    for name, m in C.BWD_MODES.items():
        first = C.BWD_MODES[C.bwd_base_mode(name)]
        assert not (first["recomp"] or first["qkv_recomp"] or first["lnrep"] or first["dpre_null"]), name
        assert (first["embed"], first["pooled"]) == (m["embed"], m["pooled"]), name
    assert len({C.bwd_base_mode(name) for name in C.BWD_MODES}) == 4 < len(C.BWD_MODES)
    assert C.wt_ref(C.block_params("unit")).numel() == C.WT_TOTAL
    assert [C.grouped_ride_runs(B) for B in (1, 3, 5, 7, 8, 37)] == [False, False, False, False, True, True]
