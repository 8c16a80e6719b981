"""tests/clip_cases.py against itself: an fp32 emulation of the norm kernel's summation order lies inside the bounds on
every case, every mutant (one per mistake the tables are meant to catch) lies outside on at least one, and the tables
satisfy the launchers' preconditions.  No GPU, no native extension."""
import functools
import math

import pytest
import torch

import clip_cases as K
import wide_step_cases as C

SEED = 11


@functools.lru_cache(maxsize=None)
def _case(n, scale):
    p, g, m, v = K.clip_inputs(n, scale, SEED, slot=True)
    return p, g, m, v


def _cases():
    for n in K.CLIP_NS:
        for scale in K.CLIP_SCALES:
            g = _case(n, scale)[1]
            for gs in (1.0, 0.125):
                for name, mn in K.max_norms(g[:n], gs).items():
                    yield n, scale, gs, name, mn, g


def test_emulated_kernel_is_inside_the_bounds_on_every_case():
    worst = 0.0
    for n, scale, gs, name, mn, g in _cases():
        ref = K.clip_ref(g[:n], gs, mn)
        norm, coef = K.emulate_clip(g, n, gs, mn)
        rn, rc = K.ratio(norm - ref.norm, ref.norm_bound), K.ratio(coef - ref.coef, ref.coef_bound)
        worst = max(worst, rn, rc)
        assert K.inside(ref, norm, coef), (n, scale, gs, name, norm, ref.norm, rn, coef, ref.coef, rc)
        if name == "inactive":
            assert coef == 1.0 and ref.coef_bound == 0.0 and ref.eps_c == 0.0  # nothing but exactly 1.0 is inside
            assert not K.inside(ref, norm, 1.0 - 2.0 ** -24)
        else:
            assert 0.0 < ref.coef_bound < 1e-5 * ref.coef
        if name == "active":
            assert coef == pytest.approx(0.25, rel=1e-2)
    print("worst error / bound of the emulation: %.3f" % worst)


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_every_mutant_is_outside_the_bounds_on_some_case(mutant):
    caught = []
    for n, scale, gs, name, mn, g in _cases():
        ref = K.clip_ref(g[:n], gs, mn)
        norm, coef = K.emulate_clip(g, n, gs, mn, mutant=mutant)
        if not K.inside(ref, norm, coef):
            caught.append((n, scale, gs, name))
    print("%s: outside on %d cases, e.g. %s" % (mutant, len(caught), caught[:3]))
    assert caught, mutant


def test_missing_eps_shows_on_the_smallest_tabular_case():
    """n = 3 at the tabular scale: the norm is ~1e-3, so the 1e-6 moves the coefficient by ~0.1 %, thousands of bounds."""
    g = _case(3, "tabular")[1]
    mn = K.max_norms(g[:3], 1.0)["active"]
    ref = K.clip_ref(g[:3], 1.0, mn)
    _, coef = K.emulate_clip(g, 3, 1.0, mn, mutant="no_eps")
    assert abs(coef - ref.coef) > 100 * ref.coef_bound


def test_depth_counts_the_kernel_constants():
    assert K.clip_grid(3) == 1 and K.clip_grid(1037) == 2 and K.clip_grid(4096) == 4
    assert K.clip_grid(K.CLIP_N_TWO_PASSES) == K.CLIP_MAX_GRID
    # one pass: 1 + 2 + 1 + 6 + 3 + 1 + 6; the capped grid's second pass and its four partials per lane
    assert K.clip_depth(4096) == 20 and K.clip_depth(K.CLIP_N_TWO_PASSES) == 2 + 2 + 1 + 6 + 3 + 4 + 6
    assert K.clip_depth(K.CLIP_N_TWO_PASSES) + 1 <= 32  # what SECOND_ORDER covers
    assert K.first_pass_elems(K.CLIP_N_TWO_PASSES) == 4 * K.CLIP_MAX_GRID * K.CLIP_BLOCK
    assert K.first_pass_elems(4099) == 4096 and K.first_pass_elems(3) == 0


def test_inputs_scale_the_tail_and_the_second_pass():
    n = K.CLIP_N_TWO_PASSES
    base = C.adam_inputs(n, "unit", SEED)[1]
    g = _case(n, "unit")[1]
    fp = K.first_pass_elems(n)
    assert torch.equal(g[:fp], base[:fp]) and torch.equal(g[fp:n], base[fp:] * 10.0) and float(g[n]) == K.PAST_N
    g3 = _case(3, "unit")[1]
    assert torch.equal(g3[:3], C.adam_inputs(3, "unit", SEED)[1] * 10.0)


def test_tables_satisfy_the_launchers_preconditions():
    """n > 0, every buffer a launch is given starts 16-byte aligned (the case tensors are whole allocations, never
    offset views), max_norm and the value clamp positive and finite in fp32."""
    for n in list(K.CLIP_NS) + [K.CLIP_ADAM_N_TWO_PASSES]:
        assert n > 0
    assert K.CLIP_ADAM_N_TWO_PASSES > 4 * 2048 * 256 and K.CLIP_ADAM_N_TWO_PASSES % 4 == 3
    assert K.clip_depth(K.CLIP_ADAM_N_TWO_PASSES) + 1 <= 32  # what SECOND_ORDER covers
    for hp in K.CLIP_HYPERS:
        assert hp.grad_scale > 0 and hp.decoupled in (0, 1)
    assert K.CLIP_ADAM_BIG_HYPER in K.CLIP_HYPERS and K.CLIP_ADAM_BIG_SCALE in K.CLIP_SCALES
    for n in K.CLIP_NS:
        for scale in K.CLIP_SCALES:
            for x in _case(n, scale):
                assert x.is_contiguous() and x.dtype == torch.float32 and x.storage_offset() == 0
                assert x.data_ptr() % 16 == 0
            g = _case(n, scale)[1]
            assert g.numel() == n + 1 and float(g[n]) == K.PAST_N
            for mn in K.max_norms(g[:n], 1.0).values():
                assert 0.0 < mn < 3.4e38 and math.isfinite(mn)
            assert K.value_clip(g[:n], K.VALUE_GRAD_SCALE) > 0.0


def test_clipped_adam_reference_widens_with_the_coefficient_error():
    """The widened bound is adam_ref's plus something positive wherever the gradient matters, and a coefficient off by
    1 % lands outside it."""
    n = 4099
    p, g, m, v = (x[:n] for x in _case(n, "unit"))
    hp = K.CLIP_HYPERS[1]
    mn = K.max_norms(g, hp.grad_scale)["active"]
    cref = K.clip_ref(g, hp.grad_scale, mn)
    ref = K.clipped_adam_ref(p, g, m, v, 1, hp, cref)
    plain = C.adam_ref(p, g, m, v, 1, hp._replace(grad_scale=hp.grad_scale * cref.coef))
    assert bool((ref.m_bound > plain.m_bound).all()) and bool((ref.p_bound >= plain.p_bound).all())
    off = C.adam_ref(p, g, m, v, 1, hp._replace(grad_scale=hp.grad_scale * cref.coef * 1.01))
    assert bool(((off.m - ref.m).abs() > ref.m_bound).any())
    unclipped = C.adam_ref(p, g, m, v, 1, hp)
    assert bool(((unclipped.p - ref.p).abs() > ref.p_bound).any())


def test_clamp_before_the_scaling_is_outside_the_value_reference():
    n = 4099
    p, g, m, v = (x[:n] for x in _case(n, "unit"))
    hp = C.Hyper(C.LR, C.B1, C.B2, C.EPS, 0.0, K.VALUE_GRAD_SCALE, 0)
    c = K.value_clip(g, hp.grad_scale)
    ref = K.value_adam_ref(p, g, m, v, 1, hp, c)
    wrong = K.value_adam_ref(p, g, m, v, 1, hp, c, clamp_first=True)
    assert bool(((wrong.m - ref.m).abs() > ref.m_bound).any()) and bool(((wrong.p - ref.p).abs() > ref.p_bound).any())
    clamped = float(((g.double() * hp.grad_scale).abs() > c).double().mean())
    assert 0.3 < clamped < 0.7
    # fp32 evaluation of the clamp-after-scaling path sits inside the reference's bounds
    g32 = (g * torch.tensor(hp.grad_scale)).clamp(-c, c)
    m32 = torch.tensor(C.B1) * m + (torch.tensor(1.0) - torch.tensor(C.B1)) * g32
    assert bool(((m32.double() - ref.m).abs() <= ref.m_bound).all())
