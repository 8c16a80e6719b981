"""tests/accum_cases.py checks itself (no GPU): its fp64 reference is torch's own accumulation loop, an fp32 emulation
of the kernel's slot order lies inside the bound, and every wrong implementation lies outside it on these very inputs -
in every variant and window where it computes something different."""
import pytest
import torch
import torch.nn.functional as F

import accum_cases as ac
import infer_cases as ic
import wloss_cases as wc

IDS = [ac.case_id(c) for c in ac.CASES]
ALL = [(c, v, w) for c in ac.CASES for v in ac.VARIANTS for w in ac.windows(c)]
ALL_IDS = ["%s-%s-w%d" % (ac.case_id(c), v, w) for c, v, w in ALL]


def _forward(dims, p, x):
    a = x.to(p.dtype)
    layers = ic.split_params(p, dims)
    for l, (W, b) in enumerate(layers):
        a = a @ W.t() + b
        if l < len(layers) - 1:
            a = torch.relu(a)
    return a


def test_the_cases_have_the_windows_the_module_describes():
    assert [ac.n_windows(c) for c in ac.CASES] == [3, 2, 2, 2]
    assert [ac.micro_rows(c, ac.n_windows(c) - 1) for c in ac.CASES] == [[1, 0], [40, 5, 0], [65, 5], [17, 5, 0, 0]]
    assert [ac.n_live(c, ac.n_windows(c) - 1) for c in ac.CASES] == [1, 2, 2, 2]
    for c in ac.CASES:
        assert c[2] * -(-c[1] // ac.R) <= 256  # inside the slot cap


@pytest.mark.parametrize("case,variant,window", ALL, ids=ALL_IDS)
def test_reference_is_torchs_accumulation_loop(case, variant, window):
    """F.cross_entropy(...) / K, .backward() once per live micro-batch, in fp64."""
    dims, B, K = case
    w, eps = ac.variant_args(variant, dims[-1])
    p = ac.inputs(case)["p"].double().requires_grad_()
    last = None
    for kb in range(K):
        x, y = ac.micro_batch(case, window, kb)
        if len(y) == 0:
            continue
        last = F.cross_entropy(_forward(dims, p, x), y, weight=None if w is None else w.double(), label_smoothing=eps)
        (last / K).backward()
    ref = ac.reference(case, variant, window)
    assert torch.allclose(p.grad, ref["grads"], rtol=1e-10, atol=1e-13)
    assert abs(float(last.detach()) - ref["loss"]) < 1e-12
    assert torch.allclose(torch.stack(ref["g_kb"]).sum(0) / K, ref["grads"], rtol=0, atol=1e-15)


def _emulate(case, variant, window):
    """fp32, in the kernel's order: per tile of 32 rows a partial gradient (plain: rows already carry 1 / bs;
    weighted: un-normalised, with the tile's sum of w[y]), slots kb * T + tile summed in ascending index, then the
    fold's division(s)."""
    dims, B, K = case
    C = dims[-1]
    w, eps = ac.variant_args(variant, C)
    weighted = variant == "ws"
    w32 = torch.ones(C) if w is None else w
    p0 = ac.inputs(case)["p"]
    T = -(-B // ac.R)
    slots, wsum, lsum = [], [], []
    for kb in range(K):
        x, y = ac.micro_batch(case, window, kb)
        bs = len(y)
        for t in range(T):
            xs, ys = x[t * ac.R:(t + 1) * ac.R], y[t * ac.R:(t + 1) * ac.R]
            if len(ys) == 0:
                slots.append(torch.zeros_like(p0))
                wsum.append(torch.zeros(()))
                lsum.append(torch.zeros(()))
                continue
            p = p0.clone().requires_grad_()
            z = _forward(dims, p, xs)
            num, _, dz = wc.row_terms(z.detach(), ys, w32, eps)
            z.backward(dz if weighted else dz * (torch.ones((), dtype=torch.float32) / bs))
            slots.append(p.grad.detach())
            wsum.append(w32[ys].sum())
            lsum.append(num.sum())
    g = torch.zeros_like(p0)
    if weighted:
        for kb in range(K):
            gk, W = torch.zeros_like(p0), torch.zeros(())
            for t in range(T):
                gk = gk + slots[kb * T + t]
                W = W + wsum[kb * T + t]
            if W > 0:
                g = g + gk / W
    else:
        for s in slots:
            g = g + s
    g = g / torch.tensor(float(K))
    kb = ac.n_live(case, window) - 1
    l = sum(lsum[kb * T: (kb + 1) * T], torch.zeros(()))
    den = sum(wsum[kb * T: (kb + 1) * T], torch.zeros(())) if weighted else torch.tensor(float(ac.micro_rows(case, window)[kb]))
    assert g.dtype == torch.float32 and l.dtype == torch.float32
    return dict(grads=g, loss=float(l / den))


@pytest.mark.parametrize("case,variant,window", ALL, ids=ALL_IDS)
def test_fp32_emulation_of_the_slot_order_is_inside_the_bound(case, variant, window):
    got = _emulate(case, variant, window)
    ref = ac.reference(case, variant, window)
    print("worst |error| / bound %.4f, loss diff %.3e" % (ac.excess(got, ref), abs(got["loss"] - ref["loss"])))
    assert ac.grads_inside(got, ref) == (True, True)


@pytest.mark.parametrize("mutant", ac.MUTANTS)
@pytest.mark.parametrize("case,variant,window", ALL, ids=ALL_IDS)
def test_mutants_are_outside_the_bound(case, variant, window, mutant):
    ref = ac.reference(case, variant, window)
    bad = ac.reference(case, variant, window, mutant)
    inside = ac.grads_inside(dict(grads=bad["grads"], loss=bad["loss"]), ref)
    if not ac.mutant_differs(case, variant, window, mutant):
        assert inside == (True, True)  # the same computation here: nothing to reject
        return
    want = (True, False) if mutant == "first_loss" else (False, True)
    assert inside == want, (inside, ac.excess(dict(grads=bad["grads"]), ref), bad["loss"] - ref["loss"])


def test_every_mutant_is_rejected_somewhere():
    for mutant in ac.MUTANTS:
        hits = [(ac.case_id(c), v, w) for c, v, w in ALL if ac.mutant_differs(c, v, w, mutant)]
        assert len(hits) >= 2, mutant
