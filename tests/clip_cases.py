"""Gradient clipping as tables of cases, with fp64 references and counted error bounds.

The norm kernel (csrc/optim.hip grad_clip_coef_kernel: the global L2 norm of the flat gradient and the clip coefficient,
both left on the device) and the flat Adam step that reads the coefficient or clamps by value (adam_flat_clip_kernel,
csrc/adam_impl.h).  Every reference is float64 on the CPU from the fp32 inputs; every bound is counted from the fp32
operations of the kernel it bounds, u = 2^-24 per rounding, as in tests/wide_step_cases.py, whose inputs, Adam
reference and constants this module builds on.  tests/test_clip_cases_cpu.py runs an fp32 emulation of the kernel's
summation order, and one mutant per mistake the tables are meant to catch, against the bounds;
tests/test_grad_clip_gpu.py launches the kernels.

A plain module, not a conftest: the tests import it."""
import math
from collections import namedtuple

import numpy as np
import torch

from wide_step_cases import ADAM_N_TWO_PASSES, B1, B2, EPS, LR, SECOND_ORDER, TINY, U, Hyper, adam_inputs, adam_ref, f32

# ------------------------------------------------------------------------------------------------ the kernel's shape
CLIP_BLOCK = 256     # threads of a workgroup (optim.hip CLIP_BLOCK)
CLIP_MAX_GRID = 256  # workgroups of a launch at most (optim.hip CLIP_MAX_GRID)
WAVE = 64
CLIP_EPS = 1e-6      # torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6)


def clip_grid(n):
    """Workgroups of the launch: one per 256 float4s, 1 .. CLIP_MAX_GRID (a function of n alone)."""
    return min(max(-(-(n >> 2) // CLIP_BLOCK), 1), CLIP_MAX_GRID)


def first_pass_elems(n):
    """Elements the first grid-stride pass covers (a float4 per thread); the float4s past it take further passes."""
    return min(4 * clip_grid(n) * CLIP_BLOCK, (n >> 2) << 2)


CLIP_N_TWO_PASSES = 4 * CLIP_MAX_GRID * CLIP_BLOCK + 4 * 300 + 3  # 256 workgroups, a second pass of 300 float4s, tail 3
# n -> what it is the edge of
CLIP_NS = {
    3: "tail only: no float4 at all",
    1037: "tail 1, a partly filled second workgroup",
    4096: "whole float4s, no tail",
    4099: "n % 4 == 3: three tail elements, summed by workgroup 0",
    CLIP_N_TWO_PASSES: "the capped grid, a second grid-stride pass of 300 float4s, tail 3",
}
CLIP_SCALES = ["tabular", "unit"]
# max_norm = factor * the fp64 norm
MAX_NORM_FACTORS = {"active": 0.25, "inactive": 1e30, "boundary": 1.0}
PAST_N = 1e3  # the value of a slot past n (the executor's loss slot g[P]): a norm that reads it is far outside


def clip_depth(n):
    """The most fp32 additions a squared term passes through on its way into the sum:
      thread   one per grid-stride pass (its float4 component's accumulator), 2 for (x + y) + (z + w), 1 for the tail
      wave     6 (xor butterfly 32 .. 1)
      group    3 (four wave sums through LDS, in order)
      grid     ceil(grid / 64) (lane l adds partials l, l + 64, ..) and the butterfly's 6."""
    grid = clip_grid(n)
    passes = -(-(n >> 2) // (grid * CLIP_BLOCK))
    return passes + 2 + 1 + 6 + (CLIP_BLOCK // WAVE - 1) + -(-grid // WAVE) + 6


def clip_inputs(n, scale, seed, slot=False):
    """p, g, m, v of wide_step_cases.adam_inputs with the last n % 4 elements of g and the elements past the first
    grid-stride pass ten times as large: a dropped tail or a dropped pass moves the norm far outside the bound.
    ``slot``: g has n + 1 entries, g[n] = PAST_N (p, m, v keep n)."""
    p, g, m, v = adam_inputs(n, scale, seed)
    g = g.clone()
    g[first_pass_elems(n):] *= 10.0  # (the tail lies past the first pass too)
    if slot:
        g = torch.cat([g, torch.tensor([PAST_N])]).float()
    return p, g, m, v


ClipRef = namedtuple("ClipRef", "norm coef norm_bound coef_bound eps_c sumsq sumsq_bound")


def clip_ref(g, grad_scale, max_norm):
    """{norm, coef} of the fp32 gradient g in fp64: norm = |grad_scale| sqrt(sum g^2), coef = min(max_norm / (norm +
    1e-6), 1), with grad_scale, max_norm and 1e-6 rounded to fp32 first, as the kernel sees them.

    Bounds.  Each square is one rounding and then passes through at most d = clip_depth(n) additions, every one a
    rounding of a partial sum of non-negative terms, so |S^ - S| <= (d + 1) u S SECOND_ORDER + n TINY.  The norm is
    the square root of that interval (monotone), then sqrtf's rounding and the product with |grad_scale|: 2 u more.
    The coefficient is the quotient over that interval, then the addition's and the division's roundings: 2 u more:
    the computed quotient lies in [c - bc, c + bc].  min(., 1) is monotone and 1-Lipschitz, so the computed coefficient
    lies in [min(c - bc, 1), min(c + bc, 1)] and coef_bound is the larger distance of the two ends from min(c, 1): 0
    once c - bc >= 1, where the kernel must return exactly 1.0.  eps_c: coef_bound relative to coef."""
    n = g.numel()
    gs, mn, e6 = abs(f32(grad_scale)), f32(max_norm), f32(CLIP_EPS)
    S = float((g.double() ** 2).sum())
    bS = (clip_depth(n) + 1) * U * S * SECOND_ORDER + n * TINY
    root = math.sqrt(S)
    norm = gs * root
    root_err = max(math.sqrt(S + bS) - root, root - math.sqrt(max(S - bS, 0.0)))
    bn = gs * root_err + 2 * U * norm * SECOND_ORDER + 2 * TINY
    c = mn / (norm + e6)
    c_err = max(mn / (max(norm - bn, 0.0) + e6) - c, c - mn / (norm + bn + e6))
    bq = c_err + 2 * U * c * SECOND_ORDER + 2 * TINY
    coef = min(c, 1.0)
    bc = max(min(c + bq, 1.0) - coef, coef - min(c - bq, 1.0))
    return ClipRef(norm, coef, bn, bc, bc / coef if coef > 0 else 0.0, S, bS)


def max_norms(g, grad_scale):
    """{name: max_norm} of MAX_NORM_FACTORS for the gradient g (fp32 values: what a launch is given)."""
    norm = abs(f32(grad_scale)) * math.sqrt(float((g.double() ** 2).sum()))
    return {name: f32(f * norm) for name, f in MAX_NORM_FACTORS.items()}


# ------------------------------------------------------------------------------------------------ fp32 emulation
def _butterfly(v):
    """wave_sum (csrc/dct_common.h) over the last axis of 64 lanes: v += v[lane ^ off], off = 32 .. 1; lane 0's sum."""
    lanes = np.arange(WAVE)
    off = WAVE // 2
    while off >= 1:
        v = (v + v[..., lanes ^ off]).astype(np.float32)
        off >>= 1
    return v[..., 0]


def emulate_clip(g, n, grad_scale, max_norm, mutant=None):
    """(norm, coef) as grad_clip_coef_kernel computes them, in numpy fp32 and in the kernel's summation order (the
    product and the addition rounded separately; the kernel may contract them into one rounding - fewer, so inside the
    same bound).  ``mutant``: one of MUTANTS, the mistake to make on purpose."""
    g = g.numpy().astype(np.float32)
    if mutant == "reads_past_n":
        n = n + 1
    g = g[:n]
    n4 = n >> 2
    grid = clip_grid(n)
    T = grid * CLIP_BLOCK
    passes = -(-n4 // T)
    if mutant == "second_pass_dropped":
        passes = min(passes, 1)
    term = (lambda x: np.abs(x)) if mutant == "abs_not_square" else (lambda x: (x * x).astype(np.float32))
    body = np.zeros(max(passes, 1) * T * 4, dtype=np.float32)
    take = min(n4 * 4, passes * T * 4)
    body[:take] = g[:take]
    body = body.reshape(-1, T, 4)
    acc = np.zeros((T, 4), dtype=np.float32)
    for k in range(body.shape[0]):
        acc = (acc + term(body[k])).astype(np.float32)
    s = ((acc[:, 0] + acc[:, 1]).astype(np.float32) + (acc[:, 2] + acc[:, 3]).astype(np.float32)).astype(np.float32)
    tail = n - 4 * n4
    if tail and mutant != "tail_dropped":
        s[:tail] = (s[:tail] + term(g[4 * n4:])).astype(np.float32)
    w = _butterfly(s.reshape(grid, CLIP_BLOCK // WAVE, WAVE))  # [grid][4] wave sums
    part = w[:, 0]
    for k in range(1, CLIP_BLOCK // WAVE):
        part = (part + w[:, k]).astype(np.float32)
    lanes = np.zeros(-(-grid // WAVE) * WAVE, dtype=np.float32)
    lanes[:grid] = part
    lanes = lanes.reshape(-1, WAVE)
    t = np.zeros(WAVE, dtype=np.float32)
    for k in range(lanes.shape[0]):
        t = (t + lanes[k]).astype(np.float32)
    total = _butterfly(t)
    norm = np.float32(abs(np.float32(grad_scale))) * np.sqrt(np.float32(total), dtype=np.float32)
    den = norm if mutant == "no_eps" else np.float32(norm + np.float32(CLIP_EPS))
    with np.errstate(over="ignore", divide="ignore"):
        c = np.float32(np.float32(max_norm) / den)
    coef = c if mutant == "not_clamped" else min(c, np.float32(1.0))
    return float(norm), float(coef)


# every one must land outside the bounds on at least one case (tests/test_clip_cases_cpu.py)
MUTANTS = ["reads_past_n", "no_eps", "not_clamped", "abs_not_square", "tail_dropped", "second_pass_dropped"]


def ratio(err, bound):
    """|error| / bound; 0 for no error at all (a bound of 0 demands exactly that), inf for any error against a 0 bound."""
    err = abs(err)
    return 0.0 if err == 0.0 else (err / bound if bound > 0.0 else float("inf"))


def inside(ref, norm, coef):
    return ratio(norm - ref.norm, ref.norm_bound) <= 1.0 and ratio(coef - ref.coef, ref.coef_bound) <= 1.0


# ------------------------------------------------------------------------------------------------ clipped Adam
CLIP_HYPERS = [Hyper(LR, B1, B2, EPS, wd, gs, dec) for wd, dec, gs in ((0.0, 0, 1.0), (0.05, 0, 0.125), (0.05, 1, 1.0))]
CLIP_STEPS = [1, 10]
# The clipped Adam launches run every size of CLIP_NS (4096: no tail, so the device scalars are read inside the float4
# loop alone) with every MAX_NORM_FACTORS name, and once the size at which ADAM's own launch (<= 2048 workgroups of 256
# float4s) takes a second grid-stride pass, as the 3.4 M-parameter tabular model does: wide_step_cases' 2048 * 256
# float4s + 300 + tail 3.  At that size the fp64 references cost ~0.2 s each, so it runs one scale and one Hyper.
CLIP_ADAM_N_TWO_PASSES = ADAM_N_TWO_PASSES
CLIP_ADAM_BIG_SCALE = "tabular"
CLIP_ADAM_BIG_HYPER = CLIP_HYPERS[1]  # coupled decay, grad_scale 0.125
VALUE_GRAD_SCALE = 0.125  # a clamp applied before the scaling instead of after it lands far outside


def clipped_adam_ref(p, g, m, v, t, hp, cref, device_counter=False):
    """adam_ref (wide_step_cases) on the gradient clipped by norm: grad_scale replaced by grad_scale * coef (fp64).
    Its bounds widened by the sensitivity to the coefficient: the kernel's grad_scale * coef carries coef's error eps_c
    and the product's rounding u, so adam_ref is evaluated at coef (1 +- (eps_c + u)) and twice the larger endpoint
    difference is added to the p, m and v bounds, per element."""
    def at(c):
        return adam_ref(p, g, m, v, t, hp._replace(grad_scale=hp.grad_scale * c), device_counter=device_counter)

    mid = at(cref.coef)
    rel = cref.eps_c + U
    lo, hi = at(cref.coef * (1.0 - rel)), at(cref.coef * (1.0 + rel))
    wide = {}
    for name in ("p", "m", "v"):
        x = getattr(mid, name)
        wide[name] = 2.0 * torch.maximum((getattr(lo, name) - x).abs(), (getattr(hi, name) - x).abs())
    return mid._replace(p_bound=mid.p_bound + wide["p"], m_bound=mid.m_bound + wide["m"],
                        v_bound=mid.v_bound + wide["v"])


def value_clip(g, grad_scale):
    """The clamp of the "value" cases: the median of |grad_scale g|, so about half the elements are clamped."""
    return f32(float((g.double() * f32(grad_scale)).abs().median()))


def value_adam_ref(p, g, m, v, t, hp, clip_value, device_counter=False, clamp_first=False):
    """adam_ref on the gradient clamped by value after scaling: clamp(grad_scale g, -c, c) in fp64, handed to adam_ref
    with grad_scale 1.  The clamp is exact in fp32 (it returns its argument or +-c), so the bounds stay adam_ref's:
    the scaling's rounding is still one of the roundings it counts.  ``clamp_first``: the mistake of clamping before
    the scaling (a mutant)."""
    gs, c = f32(hp.grad_scale), f32(clip_value)
    gc = g.double().clamp(-c, c) * gs if clamp_first else (g.double() * gs).clamp(-c, c)
    return adam_ref(p, gc, m, v, t, hp._replace(grad_scale=1.0), device_counter=device_counter)
