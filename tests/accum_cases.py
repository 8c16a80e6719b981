"""Gradient accumulation in the batch-tiled MLP trainer (csrc/mlp_tile.hip, MlpArgs::accum): the cases the GPU tests
run, their fp64 reference, the bound, and the wrong implementations the bound must reject.

Lightning 2.1's ``accumulate_grad_batches = K`` under automatic optimization: a rank's epoch is its batches
b = 0 .. nb - 1 of B rows (the last may be short), window w is batches [wK, wK + K), and the optimizer step of a window
applies

    g = (1 / K) * sum_kb grad(loss_kb)        over the window's live micro-batches - always 1 / K, also in a short window

with ``loss_kb`` the micro-batch's OWN mean (over its own row count; weighted: over its own W_kb = sum_i w[y_i]).  The
loss reported for the step is the unscaled loss of the window's last live micro-batch.

``CASES``: (dims, B, K), the smallest shapes at which the window logic can go wrong, each over
``n_items = (K + 1) B + 5`` index entries built with tests/wloss_cases.py's imbalanced-label recipe.  Window 0 is full.
For B > 5 there are two windows and the last holds one full micro-batch, one of 5 rows and K - 2 dead ones; at B = 4
the 5 extra rows are one more full batch and one row, so there are three windows at K = 2 and the last holds a
micro-batch of 1 row and a dead one.  ``_check_structure`` asserts this on import.

``VARIANTS``: "plain" (no weights, no smoothing) and wloss_cases' "ws" (class weights and smoothing).

``reference(case, variant, window, mutant=None)``: fp64 from the case's fp32 inputs, through wloss_cases' fp64 MLP and
row terms - torch's cross-entropy is not part of it (tests/test_accum_cases_cpu.py compares the two).

Bound per gradient element: ``GRAD_ATOL + GRAD_RTOL * (1 / K) sum_kb |g_kb|``.  Every micro-batch's gradient is a
result the project's per-batch check accepts inside ``GRAD_ATOL + GRAD_RTOL |g_kb|``; the mean of K such results is
inside the mean of their bounds, and the K-term sum and the division add a few units of 2^-24 of values the same bound
dominates.  (``|sum_kb g_kb / K|`` in place of the mean of the magnitudes would be too tight where the micro-batches'
gradients cancel.)  The loss is one micro-batch's: ``LOSS_ATOL``.  All three constants are wloss_cases'.

A plain module, not a conftest: the tests import it."""
import functools

import torch

import infer_cases as ic
import wloss_cases as wc

R = wc.R
CASES = [([5, 64, 2], 4, 2), ([5, 64, 2], 40, 3), ([7, 48, 32, 3], 65, 2), ([32, 128, 128, 4], 17, 4)]
VARIANTS = {"plain": (False, 0.0), "ws": wc.VARIANTS["ws"]}  # name -> (class weights on, eps)
GRAD_ATOL, GRAD_RTOL, LOSS_ATOL = wc.GRAD_ATOL, wc.GRAD_RTOL, wc.LOSS_ATOL
# div_by_live: divides by the live micro-batches; no_div: the plain sum; one_big_batch: the window as ONE batch (its
# total rows, or in "ws" one W over the window); first_loss: reports the first micro-batch's loss; norm_by_B: a short
# micro-batch's mean taken over B rows (in "ws": over W_kb * B / bs)
MUTANTS = ["div_by_live", "no_div", "one_big_batch", "first_loss", "norm_by_B"]


def case_id(case):
    dims, B, K = case
    return ic.name(dims) + f"-b{B}-k{K}"


def n_items_of(case):
    dims, B, K = case
    return (K + 1) * B + 5


def n_batches(case):
    return -(-n_items_of(case) // case[1])


def n_windows(case):
    return -(-n_batches(case) // case[2])


def windows(case):
    """The windows the one-step checks run: the full first one and the last."""
    return (0, n_windows(case) - 1)


def micro_rows(case, window):
    """Row counts of the window's K micro-batches (0: dead)."""
    dims, B, K = case
    n = n_items_of(case)
    return [max(0, min(B, n - (window * K + kb) * B)) for kb in range(K)]


def n_live(case, window):
    return sum(1 for bs in micro_rows(case, window) if bs > 0)


def variant_args(variant, C):
    """(class weights fp32 [C] or None, eps) of a variant."""
    on, eps = VARIANTS[variant]
    return (wc.class_weights(C) if on else None), eps


def inputs(case):
    """The case's fp32 / integer inputs on the CPU (wloss_cases.inputs with K + 1 full batches and 5 rows): p, X, Y,
    idx int32 [n_items_of(case)]."""
    dims, B, K = case
    return wc.inputs((dims, B), K + 1)


def micro_batch(case, window, kb):
    """(x fp32 [bs, D0], y int64 [bs]) of micro-batch kb of a window, in batch order (bs may be 0)."""
    dims, B, K = case
    d = inputs(case)
    b = window * K + kb
    sel = d["idx"][b * B: (b + 1) * B].long()
    return d["X"][sel], d["Y"][sel].long()


def _check_structure():
    for case in CASES:
        dims, B, K = case
        assert inputs(case)["idx"].numel() == n_items_of(case)
        assert micro_rows(case, 0) == [B] * K  # window 0 is full
        last = micro_rows(case, n_windows(case) - 1)
        if B > 5:
            assert n_windows(case) == 2 and last == [B, 5] + [0] * (K - 2)
        else:
            assert B == 4 and K == 2 and n_windows(case) == 3 and last == [1, 0]


_check_structure()


def mutant_differs(case, variant, window, mutant):
    """The mutant computes something else than the feature in this variant and window."""
    dims, B, K = case
    rows = micro_rows(case, window)
    short = any(0 < bs < B for bs in rows)
    if mutant == "div_by_live":
        return n_live(case, window) < K
    if mutant == "no_div":
        return True
    if mutant == "one_big_batch":
        # K live micro-batches with one common normaliser (plain: B rows each; "ws": labels that happen to give every
        # micro-batch the same W_kb, as at batch 4): sum_kb (1 / W) sum_rows / K is the big batch's mean
        if rows != [B] * K:
            return True
        if variant != "ws":
            return False
        w = wc.class_weights(dims[-1])
        Ws = [wc.normaliser(micro_batch(case, window, kb)[1], w) for kb in range(K)]
        return max(Ws) - min(Ws) > 1e-9 * max(Ws)
    if mutant == "first_loss":
        return n_live(case, window) > 1
    if mutant == "norm_by_B":
        return short
    raise KeyError(mutant)


@functools.lru_cache(maxsize=None)
def _reference(dims, B, K, variant, window, mutant):
    case = (list(dims), B, K)
    C = dims[-1]
    w, eps = variant_args(variant, C)
    w = torch.ones(C) if w is None else w
    p0 = inputs(case)["p"]
    P = p0.numel()
    g_kb, losses, raw, Ws, ns = [], [], [], [], []
    for kb in range(K):
        x, y = micro_batch(case, window, kb)
        if len(y) == 0:
            g_kb.append(torch.zeros(P, dtype=torch.float64))
            raw.append(torch.zeros(P, dtype=torch.float64))
            Ws.append(0.0)
            ns.append(0)
            continue
        p = p0.double().requires_grad_()
        z = wc.forward64(list(dims), p, x)
        num, t, dz = wc.row_terms(z.detach(), y, w.double(), eps)
        W = wc.normaliser(y, w)  # plain: w = 1, W = the micro-batch's own row count
        z.backward(dz)
        raw.append(p.grad.detach().clone())  # before the normaliser
        Wm = W * B / len(y) if mutant == "norm_by_B" else W
        g_kb.append(raw[-1] / Wm)
        losses.append(float(num.sum() / W))
        Ws.append(W)
        ns.append(len(y))
    live = len(losses)
    total = torch.stack(g_kb).sum(0)
    if mutant == "div_by_live":
        grads = total / live
    elif mutant == "no_div":
        grads = total
    elif mutant == "one_big_batch":
        grads = torch.stack(raw).sum(0) / sum(Ws)
    else:
        grads = total / K
    loss = losses[0] if mutant == "first_loss" else losses[-1]
    mag = torch.stack([g.abs() for g in g_kb]).sum(0) / K
    return dict(g_kb=g_kb, grads=grads, loss=loss, mag=mag, losses=losses, W=Ws, rows=ns)


def reference(case, variant, window, mutant=None):
    """fp64: dict(g_kb: K gradients [P] (zeros for a dead micro-batch), grads = sum g_kb / K [P], loss = the last live
    micro-batch's, mag = (1 / K) sum |g_kb| (the bound's magnitude), losses, W, rows per live micro-batch)."""
    dims, B, K = case
    return _reference(tuple(dims), B, K, variant, window, mutant)


def bound(ref):
    """Per-element gradient bound of a (mutant-free) reference."""
    return GRAD_ATOL + GRAD_RTOL * ref["mag"]


def grads_inside(got, ref):
    """The grad-mode check of the GPU test: (gradients inside, loss inside)."""
    err = (got["grads"].double() - ref["grads"]).abs()
    return bool((err <= bound(ref)).all()), abs(float(got["loss"]) - ref["loss"]) < LOSS_ATOL


def excess(got, ref):
    """Worst |error| / bound over the gradient (<= 1 passes), for printing."""
    return float(((got["grads"].double() - ref["grads"]).abs() / bound(ref)).max())
