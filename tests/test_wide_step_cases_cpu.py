"""tests/wide_step_cases.py against itself: every fp64 reference, rounded to the kernel's output format, lies inside
its own bound (so a GPU failure is the kernel's, not the inputs'), a plain fp32 evaluation of adam_one does too, the
gather reference wraps as csrc/kernels.h says, and every table row satisfies its launcher's preconditions and names
the kernel it is meant to reach.  No GPU."""
import numpy as np
import pytest
import torch

import wide_step_cases as C


def _parts(case, scale, seed=11):
    _, n, ranges, _ = case
    return [(off, cnt, sp, s) for (off, cnt, sp), s in zip(ranges, C.part_slices(ranges, scale, seed))]


def _fp32_adam(p, g, m, v, t, hp, parts):
    """adam_one op by op in numpy float32 (no fused multiply-add), host-t bias corrections."""
    f = np.float32
    p, g, m, v = (x.numpy().astype(f) for x in (p, g, m, v))
    g = g.copy()
    for off, cnt, sp, s in parts or []:
        acc = s[0].numpy().astype(f)
        for q in range(1, sp):
            acc = acc + s[q].numpy().astype(f)
        g[off:off + cnt] = acc
    lr, b1, b2, eps, wd, gs = (f(x) for x in (hp.lr, hp.b1, hp.b2, hp.eps, hp.wd, hp.grad_scale))
    ss, rbc2, _, _ = C.bias_corrections(hp, t, False)
    g = g * gs
    if hp.decoupled:
        p = p - lr * wd * p
    else:
        g = g + wd * p
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * g * g
    p = p - f(ss) * m / (np.sqrt(v) * f(rbc2) + eps)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(v)


def _inside(got, want, bound):
    return float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("scale", ["tabular", "unit"])
@pytest.mark.parametrize("n", [n for n in C.ADAM_NS if n < 100000])
def test_adam_reference_and_a_plain_fp32_evaluation_lie_inside_the_bounds(n, scale):
    p, g, m, v = C.adam_inputs(n, scale, seed=n)
    worst = 0.0
    for hp in C.HYPERS:
        for t in C.STEPS:
            ref = C.adam_ref(p, g, m, v, t, hp)
            assert torch.isfinite(ref.p).all() and (ref.m_bound > 0).all() and (ref.v_bound > 0).all()
            for name, r, b in (("p", ref.p, ref.p_bound), ("m", ref.m, ref.m_bound), ("v", ref.v, ref.v_bound)):
                assert _inside(r.float(), r, b) <= 1.0, (name, hp, t)
            mirror = _fp32_adam(p, g, m, v, t, hp, None)
            for name, got, r, b in zip("pmv", mirror, (ref.p, ref.m, ref.v), (ref.p_bound, ref.m_bound, ref.v_bound)):
                ratio = _inside(got, r, b)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, hp, t, ratio)
            # the device-counter bound only adds to the host one, and the two references differ by the casts alone
            dev = C.adam_ref(p, g, m, v, t, hp, device_counter=True)
            assert (dev.p_bound >= ref.p_bound).all()
            assert _inside(dev.p, ref.p, 2 * C.U * ref.upd.abs() + 1e-300) <= 1.0
    print("worst fp32-evaluation error / bound %.3f" % worst)


@pytest.mark.parametrize("scale", ["tabular", "unit"])
@pytest.mark.parametrize("case", C.PARTS_CASES, ids=[c[0] for c in C.PARTS_CASES])
def test_parts_reference_sums_the_slices_and_lies_inside_its_bounds(case, scale):
    _, n, ranges, _ = case
    p, g, m, v = C.adam_inputs(n, scale, seed=5)
    parts = _parts(case, scale)
    g_nan = g.clone()
    for off, cnt, _ in ranges:
        g_nan[off:off + cnt] = float("nan")
    for hp in C.HYPERS:
        ref = C.adam_ref(p, g_nan, m, v, 10, hp, parts=parts)
        assert all(torch.isfinite(x).all() for x in ref), "the canaries leak into the reference"
        # the same as handing Adam the summed gradient
        gsum = g.clone().double()
        for off, cnt, sp, s in parts:
            gsum[off:off + cnt] = s[:sp].double().sum(0)
        flat = C.adam_ref(p, gsum.float(), m, v, 10, hp)
        assert _inside(ref.m, flat.m, flat.m_bound) <= 1.0 and _inside(ref.p, flat.p, flat.p_bound) <= 1.0
        mirror = _fp32_adam(p, g, m, v, 10, hp, parts)
        for name, got, r, b in zip("pmv", mirror, (ref.p, ref.m, ref.v), (ref.p_bound, ref.m_bound, ref.v_bound)):
            assert _inside(got, r, b) <= 1.0, (name, hp)


def test_adam_reference_leaves_elements_outside_the_range_unchanged():
    p, g, m, v = C.adam_inputs(C.RANGE_N, "unit", seed=2)
    full = C.adam_ref(p, g, m, v, 3, C.HYPERS[3])
    for lo, hi in C.RANGES:
        r = C.adam_ref(p, g, m, v, 3, C.HYPERS[3], lo=lo, hi=hi)
        out = torch.ones(C.RANGE_N, dtype=torch.bool)
        out[lo:hi] = False
        assert torch.equal(r.p[out], p.double()[out]) and torch.equal(r.m[out], m.double()[out])
        assert torch.equal(r.v[out], v.double()[out]) and (r.p_bound[out] == 0).all()
        assert torch.equal(r.p[lo:hi], full.p[lo:hi]) and torch.equal(r.v[lo:hi], full.v[lo:hi])


def test_gather_rows_reference_wraps_inside_the_item_list():
    idx = torch.tensor([10, 11, 12, 13, 14, 15, 16, 99, 98], dtype=torch.int32)  # 7 items, then entries never read
    # cursor 1, stride 4, 6 rows: q = 4, 5, 6, 7 -> 0, 8 -> 1, 9 -> 2
    assert C.gather_rows_ref(idx, 1, 4, 7, 6).tolist() == idx.long()[[4, 5, 6, 0, 1, 2]].tolist() == [14, 15, 16, 10, 11, 12]
    assert C.gather_rows_ref(idx, 0, 4, 7, 4).tolist() == [10, 11, 12, 13]
    assert C.gather_rows_ref(idx, 5, 4, 7, 3).tolist() == [16, 10, 11]  # q = 20, 21, 22: more than one lap
    for M in (1, 50, 128, 2100):
        stride, n_items, n_idx, cursors = C.batch_geometry(M)
        assert cursors == (0, 2) and n_idx >= cursors[1] * stride + M
        assert cursors[0] * stride + M <= n_items < cursors[1] * stride + M  # inside / the last rows wrap
        q = cursors[1] * stride + torch.arange(M)
        assert (C.gather_rows_ref(torch.arange(n_idx), 2, stride, n_items, M) != q)[q >= n_items].all()


def test_gemm_references_rounded_to_the_output_format_lie_inside_their_bounds():
    gen = torch.Generator().manual_seed(0)
    M, N, K = 40, 24, 128
    a = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    b = (torch.randn(K, N, generator=gen) * 0.1).to(torch.bfloat16)
    ref, ab = C.gemm_ref(a, b)
    assert (ab >= ref.abs()).all()
    assert _inside(ref.float(), ref, C.partial_bound(ref, ab, K)) <= 1.0
    assert _inside(a.float() @ b.float(), ref, C.partial_bound(ref, ab, K)) <= 1.0  # an fp32 product
    z = ref + torch.randn(N, generator=gen).double()
    assert _inside(z.to(torch.bfloat16), z, C.fwd_bound(z, ab, K)) <= 1.0
    assert _inside(z.clamp_min(0).to(torch.bfloat16), z.clamp_min(0), C.fwd_bound(z, ab, K)) <= 1.0
    gz = C.gelu_ref(z)
    assert _inside(gz.to(torch.bfloat16), gz, C.gelu_out_bound(z, ab, K)) <= 1.0
    assert _inside(torch.nn.functional.gelu(z.float()).to(torch.bfloat16), gz, C.gelu_out_bound(z, ab, K)) <= 1.0
    zz = torch.linspace(-6, 6, 2001, dtype=torch.float64).requires_grad_()
    (slope,) = torch.autograd.grad(C.gelu_ref(zz).sum(), zz)
    assert 1.12 < float(slope.abs().max()) <= C.GELU_LIP


def test_adam_tables_satisfy_the_launchers_preconditions():
    assert sorted(n % 4 for n in C.ADAM_NS) == [0, 0, 1, 3, 3] and max(C.ADAM_NS) == 600000
    assert C.ADAM_N_TWO_PASSES // 4 > 2048 * 256 and C.ADAM_N_TWO_PASSES % 4 == 3  # what 600000 does not reach
    assert set(C.STEPS) == {1, 2, 10, 1000} and len(C.HYPERS) == 6
    assert {(h.wd, h.decoupled) for h in C.HYPERS} == {(0.0, 0), (0.05, 0), (0.05, 1)}
    assert {h.grad_scale for h in C.HYPERS} == {1.0, 0.125}
    kernels = set()
    for name, n, ranges, kernel in C.PARTS_CASES:
        assert n % 4 == 3 and 1 <= len(ranges) <= 3
        prev_end = 0
        for off, cnt, sp in ranges:
            assert off % 4 == 0 and cnt % 4 == 0 and off + cnt <= (n & ~3) and 1 <= sp <= C.PART_SLOTS == 8
            assert off > prev_end or (off == prev_end == 0), "ranges leave gaps that read g"
            prev_end = off + cnt
        assert kernel == "adam_flat_kernel<true, %d>" % (8 if max(sp for _, _, sp in ranges) > 4 else 4)
        kernels.add(kernel)
    assert len(kernels) == 2
    assert any(r[-1][0] + r[-1][1] == (n & ~3) for _, n, r, _ in C.PARTS_CASES), "one range ends at n & ~3"
    assert [sp for _, _, sp in C.PARTS_CASES[0][2]] == [1, 4, 8] and [sp for _, _, sp in C.PARTS_CASES[1][2]] == [2, 3, 4]
    assert [sp for _, _, sp in C.PARTS_CASES[2][2]] == [5]
    for lo, hi in C.RANGES:
        assert lo % 4 == 0 and lo < hi and (hi % 4 == 0 or hi == C.RANGE_N)
    assert C.RANGES[0][1] == C.RANGES[1][0] and C.RANGES[0][0] == 0 and C.RANGES[1][1] == C.RANGE_N and C.RANGE_N % 4
    assert set(C.ADAM_LAUNCHERS) == {"adam_flat", "adam_flat_step", "adam_flat_step_parts", "adam_range"}
    assert all("kernel" in k for k in C.ADAM_LAUNCHERS.values())


def test_gemm_tables_satisfy_the_launchers_preconditions():
    for M, N, K, splits, what in C.DW_CASES:
        nk = K // C.GBK
        assert K % C.GBK == 0 and M % 8 == 0 and N % 8 == 0 and 1 <= splits <= nk and what
        sl = C.dw_slices(K, splits)
        assert len(sl) == splits and sl[0][0] == 0 and sl[-1][1] == K and all(k1 > k0 for k0, k1 in sl)
        assert all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert (splits - 1) * -(-nk // splits) < nk
    assert any(s == 8 for _, _, _, s, _ in C.DW_CASES) and any(M % 128 and N % 128 for M, N, _, _, _ in C.DW_CASES)
    assert [k1 - k0 for k0, k1 in C.dw_slices(448, 3)] == [192, 192, 64]
    (M, N, K, s, _), (M2, N2, K2, s2, _) = C.DW_REJECTED
    assert s > K // C.GBK and s2 <= K2 // C.GBK and (s2 - 1) * -(-(K2 // C.GBK) // s2) >= K2 // C.GBK
    parts = {c[0]: c for c in C.PARTS_CASES}
    for n, pc, f4, kernel in C.RIDE_CASES:
        S = 8 if pc and max(sp for _, _, sp in parts[pc][2]) > 4 else 4
        assert kernel.startswith("gemm2_dw_adam_kernel<%d, %s>" % (S, "true" if f4 else "false"))
        assert pc is None or parts[pc][1] == n
    assert {k.split(":")[0] for _, _, _, k in C.RIDE_CASES} == {
        "gemm2_dw_adam_kernel<%d, %s>" % (S, f) for S in (4, 8) for f in ("true", "false")}
    assert any(n > 256 * 512 for n, _, _, _ in C.RIDE_CASES)

    for M, N, K, kernel, what in C.GATHER_CASES:
        assert N % 8 == 0 and K % C.GBK == 0 and what
        assert kernel == C.gather_kernel(M, N, K, 256)  # the MI355X's 256 compute units
        if kernel == C.W8:
            tiles = -(-M // 128) * -(-N // 128)
            assert tiles == 136 and K % 128 == 0 and K >= 256
            assert C.gather_kernel(M, N, K, 135) == C.W4 and C.gather_kernel(M, N, K, 272) == C.W4
    assert {k for _, _, _, k, _ in C.GATHER_CASES} == {C.W4, C.W8}
    assert -(-128 // -(-264 // 128)) == 43  # the a_out band of the three-column-tile shapes
    for M, N, K, epi, nz, what in C.GATHER_REJECTED:
        assert sum([N % 8 != 0, K % C.GBK != 0, nz > 4, epi in (C.EPI_RELU_MASK, C.EPI_GELU_GRAD)]) == 1, what


def test_zero_ranges_and_step_tables():
    mask = C.zero_mask()
    assert all(off % 4 == 0 and off + cnt <= C.ZERO_LEN for off, cnt in C.ZERO_RANGES) and len(C.ZERO_RANGES) == 4
    assert int(mask.sum()) == 7 + 4 + 1030 and not mask[7] and mask[2053] and not mask[2054] and not mask[4096]
    assert {cnt % 4 for _, cnt in C.ZERO_RANGES} == {3, 0, 2}
    assert {B for B, _ in C.STEP_CASES} == {1, 50, 4096} and {rb for _, rb in C.STEP_CASES} == {16, 512}
    assert all(rb % 16 == 0 for _, rb in C.STEP_CASES)
    assert C.ZERO_NS == [1, 3, 4, 5, (1 << 20) | 3] and (C.ZERO_NS[-1] + 3) // 4 > 2048 * 256 // 4
    assert set(C.STEP_LAUNCHERS) == {"gather_batch_step_ranges", "zero_f32", "ag_step_prologue", "step_end"}
    assert all("kernel" in k for k in C.STEP_LAUNCHERS.values())
    assert set(C.DW_KERNELS) == {"none", "scalar", "float4"} and all("kernel<" in k for k in C.DW_KERNELS.values())
    # a one-row batch of 16-byte rows is one unit of gather work: the zero range sizes that grid
    assert max(cnt for _, cnt in C.ZERO_RANGES) // 4 > 256 > 1 * 16 // 16
