"""tests/optim_cases.py against itself, without a GPU: its fp64 formulas are torch.optim.SGD's / AdamW's (stepped in
fp64 from the same state on the same gradient), an fp32 evaluation in the kernels' operation order lies inside the
derived bound for every case, variant and step count, and each of the nine wrong implementations lies outside it
somewhere."""
import pytest
import torch

import optim_cases as oc

IDS = [oc.case_id(c) for c in oc.CASES]


def _torch_step(p, g, m, v, hp, taken):
    """torch's optimizer in fp64 (hyper-parameters rounded to fp32, as the kernels get them), from the state (m, v)
    after ``taken`` steps - no state at all when taken == 0, which is what makes the first step the first."""
    q = p.double().clone().requires_grad_()
    opt = oc.torch_optimizer([q], hp)
    if taken:
        if hp.kind == "sgd":
            if hp.momentum:
                opt.state[q]["momentum_buffer"] = m.double().clone()
        else:
            opt.state[q].update(step=torch.tensor(float(taken)), exp_avg=m.double().clone(),
                                exp_avg_sq=v.double().clone())
    q.grad = g.double().clone()
    opt.step()
    st = opt.state[q]
    return q.detach(), st.get("momentum_buffer", st.get("exp_avg")), st.get("exp_avg_sq")


@pytest.mark.parametrize("taken", oc.STEP_COUNTS)
@pytest.mark.parametrize("variant", list(oc.VARIANTS))
@pytest.mark.parametrize("case", oc.CASES, ids=IDS)
def test_reference_is_torch_and_fp32_lies_inside_the_bound(case, variant, taken):
    hp = oc.VARIANTS[variant]
    p, m, v = oc.state(case, hp, taken)
    g = oc.cpu_gradient(case)
    ref = oc.reference(p, g, m, v, hp, taken)
    tp, tm, tv = _torch_step(p, g, m, v, hp, taken)
    assert torch.allclose(ref.p, tp, rtol=1e-12, atol=1e-15)
    for mine, theirs in ((ref.m, tm), (ref.v, tv)):
        assert (mine is None) == (theirs is None)
        if mine is not None:
            assert torch.isfinite(mine).all() and torch.allclose(mine, theirs, rtol=1e-12, atol=1e-18)
    got = oc.emulate_fp32(p, g, m, v, hp, taken)
    print("%s %s t=%d: fp32 emulation, worst |error| / bound %.4f" % (oc.case_id(case), variant, taken,
                                                                      oc.excess(got, ref)))
    assert oc.inside(got, ref)
    # the bound is a few units of roundoff of the terms, not a tolerance that swallows the update
    assert float((ref.p_bound / (ref.p - p.double()).abs().clamp_min(1e-30)).median()) < 1e-2


def _rejected(mutant):
    """Does some case x variant x step count put the mutant outside the bound?  (The mutant's own fp64 result, which
    an fp32 evaluation of it would track within the same bound.)"""
    for case in oc.CASES:
        g = oc.cpu_gradient(case)
        for hp in oc.VARIANTS.values():
            for taken in oc.STEP_COUNTS:
                p, m, v = oc.state(case, hp, taken)
                ref = oc.reference(p, g, m, v, hp, taken)
                bad = oc.reference(p, g, m, v, hp, taken, mutant=mutant, lr_base=oc.LR_BASE)
                got = tuple(None if x is None else x for x in (bad.p, bad.m, bad.v))
                if not oc.inside(got, ref):
                    return True
    return False


@pytest.mark.parametrize("mutant", oc.MUTANTS)
def test_every_mutant_is_rejected_somewhere(mutant):
    assert _rejected(mutant)


def test_mutants_are_rejected_by_a_margin_and_the_feature_is_not():
    """Worst |error| / bound of each mutant where it is caught is far above 1 - the bound has room to spare on the
    wrong side, none on the right one (the mutant-free reference against itself is 0)."""
    case = oc.CASES[1]
    g = oc.cpu_gradient(case)
    for mutant, variant, taken in (("first_dampened", "sgd_mdw", 0), ("nesterov_ignored", "sgd_nest", 3),
                                   ("sgd_decoupled", "sgd_mdw", 3), ("adamw_coupled", "adamw", 3),
                                   ("adamw_base_rate", "adamw", 3), ("dampening_ignored", "sgd_mdw", 3),
                                   ("momentum_on_p", "sgd_m", 3), ("nesterov_old_buf", "sgd_nest", 3)):
        hp = oc.VARIANTS[variant]
        p, m, v = oc.state(case, hp, taken)
        ref = oc.reference(p, g, m, v, hp, taken)
        bad = oc.reference(p, g, m, v, hp, taken, mutant=mutant, lr_base=oc.LR_BASE)
        assert oc.excess((bad.p, bad.m, bad.v), ref) > 100, mutant
        assert oc.excess((ref.p, ref.m, ref.v), ref) == 0.0
    # the first step's garbage buffer: a kernel that reads it produces NaNs, which no bound admits
    hp = oc.VARIANTS["sgd_m"]
    p, m, v = oc.state(case, hp, 0)
    assert torch.isnan(m).any()
    bad = oc.reference(p, g, m, v, hp, 0, mutant="first_reads_m")
    assert not oc.inside((bad.p, bad.m, bad.v), oc.reference(p, g, m, v, hp, 0))
