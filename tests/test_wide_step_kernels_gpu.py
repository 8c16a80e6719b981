"""The wide-MLP step's launchers, each on its own, element by element against the fp64 references and derived bounds of
tests/wide_step_cases.py: flat Adam on the host-t and the device-counter path (dct_adam_flat, _step, _step_parts,
dct_adam_range), the split-K dW partials with Adam riding along (dct_gemm_bf16_dw_partials_adam[_ex]), the gathered
first forward GEMM (dct_gemm_bf16_gather_fwd) and the step bookkeeping kernels (dct_gather_batch[_step_ranges],
dct_ag_step_prologue, dct_zero_f32, dct_step_end).  Every comparison is kernel against reference, never one kernel
path against another; every test prints its worst error / bound ratio before it asserts.

Measured on an MI355X (2026-10-20), b1 = 0.9, b2 = 0.999, lr = 1e-3, tabular-scale inputs (unit scale within 20 %).
Error of Adam's update in units of the update, median over 4096 elements at p = 0 (so p's own rounding hides
nothing), and the worst error / bound ratio of the same launch (test_update_error_of_the_two_bias_correction_paths):

    t       host t (double)         device counter (fp32 1 - exp2(t log2 b))     granted to bc1 + bc2
    1       4.9e-08   0.24          4.9e-08   0.04                               1.3e-06 + 1.2e-04
    2       4.7e-08   0.19          3.3e-06   0.06                               6.9e-07 + 6.0e-05
    10      4.8e-08   0.20          2.2e-07   0.06                               2.4e-07 + 1.2e-05
    1000    4.7e-08   0.21          5.1e-08   0.17                               1.8e-07 + 1.9e-07

The device path's error stays inside the cancellation term 2^-23 / (1 - b^t) at every t (worst at t = 2: 3.3e-06 of
the 6.0e-05 granted), so adam_bias_correction stays as it is.  Worst error / bound over every other case: p 0.998
(its own final rounding, u |p|, is most of that bound), m 0.43, v 0.46, dW partials 0.023, colsum 0.003, gathered
forward C 0.992 and aux 0.992 (the bf16 rounding itself: 2^-8 / (1 + 2^-8) of |z| at worst).
"""
import functools

import pytest
import torch

import wide_step_cases as C

pytestmark = pytest.mark.gpu

GUARD_I32 = -77
GUARD_BF16 = -7.0


def _nat():
    from dct_amd.ops._native import native

    return native()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev():
    return torch.device("cuda", 0)


def _ratio(what, got, want, bound):
    """Worst |got - want| / bound; <= 1 passes.  A non-finite value anywhere is reported as inf."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        print("  %s: non-finite values" % what)
        return float("inf")
    r = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
    print("  %s: worst error / bound %.4f" % (what, r))
    return r


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4
                               else torch.int64)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


class AdamState:
    """p, g, m, v (+ the bf16 shadow) on the device, each with a guard element after it."""

    def __init__(self, p, g, m, v):
        d = _dev()
        self.n = n = p.numel()
        self.init = [torch.cat([x, torch.full((1,), 123.0)]).to(d) for x in (p, g, m, v)]
        self.reset()

    def reset(self):
        self.p, self.g, self.m, self.v = (x.clone() for x in self.init)
        self.pb = torch.full((self.n + 1,), GUARD_BF16, dtype=torch.bfloat16, device=_dev())

    def ptrs(self):
        return self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.pb.data_ptr()

    def untouched(self):
        return (all(_same_bits(a, b) for a, b in zip((self.p, self.g, self.m, self.v), self.init))
                and bool((self.pb == GUARD_BF16).all()))

    def check(self, what, dref):
        """p, m, v inside their bounds; g and the guards intact; the shadow is the kernel's own p in bf16."""
        n = self.n
        assert _same_bits(self.g, self.init[1]), what + ": g changed"
        for x in (self.p, self.m, self.v):
            assert float(x[n]) == 123.0, what + ": wrote past n"
        assert float(self.pb[n]) == GUARD_BF16, what + ": the shadow wrote past n"
        rp = _ratio(what + " p", self.p[:n], dref.p, dref.p_bound)
        rm = _ratio(what + " m", self.m[:n], dref.m, dref.m_bound)
        rv = _ratio(what + " v", self.v[:n], dref.v, dref.v_bound)
        assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0, (what, rp, rm, rv)
        inside = dref.p_bound > 0
        assert _same_bits(self.pb[:n][inside], self.p[:n][inside].to(torch.bfloat16)), what + ": bf16 shadow != bf16(p)"
        assert bool((self.pb[:n][~inside] == GUARD_BF16).all()), what + ": shadow written outside the range"
        return rp


def _to_dev(ref):
    return C.AdamRef(*(x.to(_dev()) for x in ref))


def _hp_args(hp):
    return hp.lr, hp.b1, hp.b2, hp.eps, hp.wd


def _launch(nat, launcher, s, hp, t, step, n=None, parts=((), (), (), ()), lo=0, hi=None, cursor=0, slot=0, out=0,
            cap=0, ptrs=None):
    """One Adam launch.  ``step``: the device step counter (None: the host-t path)."""
    n = s.n if n is None else n
    p, g, m, v, pb = ptrs or s.ptrs()
    sc = 0 if step is None else step.data_ptr()
    if launcher == "adam_flat":
        nat.adam_flat(p, g, m, v, pb, n, *_hp_args(hp), t if step is None else 1, hp.grad_scale, hp.decoupled, sc, _st())
    elif launcher == "adam_flat_step":
        nat.adam_flat_step(p, g, m, v, pb, n, *_hp_args(hp), t if step is None else 1, hp.grad_scale, hp.decoupled,
                           sc, cursor, slot, out, cap, _st())
    elif launcher == "adam_flat_step_parts":
        nat.adam_flat_step_parts(p, g, m, v, pb, n, *_hp_args(hp), hp.grad_scale, hp.decoupled, sc, cursor, slot, out,
                                 cap, *parts, _st())
    else:
        r = nat.AdamRange(p, g, m, v, pb, n, *_hp_args(hp), hp.grad_scale, hp.decoupled, sc, *parts, lo,
                          n if hi is None else hi)
        nat.adam_range(r, cursor, slot, out, cap, _st())
    torch.cuda.synchronize()


def _step_tensor(t):
    return torch.tensor([t], dtype=torch.int32, device=_dev())


# ---------------------------------------------------------------------------------------------- (a) flat Adam
@pytest.mark.parametrize("path", ["host_t", "device_counter"])
@pytest.mark.parametrize("scale", ["tabular", "unit"])
@pytest.mark.parametrize("n", list(C.ADAM_NS))
def test_flat_adam_matches_fp64_elementwise(n, scale, path):
    """Every launcher of the path, every (wd, decoupled), grad_scale and t: p, m, v inside the derived bounds."""
    nat = _nat()
    dev_t = path == "device_counter"
    launchers = list(C.ADAM_LAUNCHERS) if dev_t else ["adam_flat", "adam_flat_step"]
    cpu = C.adam_inputs(n, scale, seed=n)
    s = AdamState(*cpu)
    for t in C.STEPS:
        worst, med = 0.0, []
        for hp in C.HYPERS:
            dref = _to_dev(C.adam_ref(*cpu, t, hp, device_counter=dev_t))
            for launcher in launchers:
                s.reset()
                _launch(nat, launcher, s, hp, t, _step_tensor(t) if dev_t else None)
                worst = max(worst, s.check("%s t=%d %s" % (launcher, t, hp), dref))
                med.append(float(((s.p[:n].double() - dref.p).abs() / dref.upd.abs().clamp_min(1e-300)).median()))
        print("UPDATE-ERROR %s %s n=%d t=%d: worst |p err| / bound %.3f, median |p err| / |update| %.2e"
              % (path, scale, n, t, worst, max(med)))


@pytest.mark.parametrize("scale", ["tabular", "unit"])
def test_update_error_of_the_two_bias_correction_paths(scale):
    """p = 0, so p' = -update exactly and nothing of p's own rounding hides the update's error: what the fp32
    1 - exp2(t log2 b) of the device-counter path costs next to the host's double (the figures in this module's
    docstring).  Both stay inside adam_ref's bound, the device path's with its cancellation term."""
    nat, n, hp = _nat(), 4096, C.HYPERS[0]
    p, g, m, v = C.adam_inputs(n, scale, seed=8)
    cpu = (torch.zeros_like(p), g, m, v)
    s = AdamState(*cpu)
    for t in C.STEPS:
        for dev_t in (False, True):
            dref = _to_dev(C.adam_ref(*cpu, t, hp, device_counter=dev_t))
            s.reset()
            _launch(nat, "adam_flat", s, hp, t, _step_tensor(t) if dev_t else None)
            rel = (s.p[:n].double() - dref.p).abs() / dref.upd.abs().clamp_min(1e-300)
            ratio = float(((s.p[:n].double() - dref.p).abs() / dref.p_bound).max())
            print("BIAS-CORRECTION %s %s t=%d: update error median %.2e worst %.2e of the update; worst error / bound "
                  "%.3f (granted: %.2e + %.2e)" % ("device" if dev_t else "host  ", scale, t, float(rel.median()),
                                                  float(rel.max()), ratio, *C.bias_corrections(hp, t, dev_t)[2:]))
            assert ratio <= 1.0, (t, dev_t, ratio)


@pytest.mark.parametrize("path", ["host_t", "device_counter"])
def test_flat_adam_second_grid_stride_pass(path):
    """More float4s than one launch's 2048 x 256 threads: the elements of the second pass and the tail after it."""
    nat, n, t = _nat(), C.ADAM_N_TWO_PASSES, 10
    dev_t = path == "device_counter"
    cpu = C.adam_inputs(n, "tabular", seed=1)
    s = AdamState(*cpu)
    for hp in (C.HYPERS[3], C.HYPERS[5]):
        dref = _to_dev(C.adam_ref(*cpu, t, hp, device_counter=dev_t))
        for launcher in (list(C.ADAM_LAUNCHERS) if dev_t else ["adam_flat"]):
            s.reset()
            _launch(nat, launcher, s, hp, t, _step_tensor(t) if dev_t else None)
            s.check("%s two passes %s" % (launcher, hp), dref)


def _part_setup(case, scale):
    """(state with NaN over the part ranges of g, device slices, launcher part arguments, reference parts)."""
    _, n, ranges, _ = case
    p, g, m, v = C.adam_inputs(n, scale, seed=5)
    for off, cnt, _ in ranges:
        g[off:off + cnt] = float("nan")
    slices = C.part_slices(ranges, scale, seed=11)
    dsl = [x.to(_dev()) for x in slices]
    args = ([r[0] for r in ranges], [r[1] for r in ranges], [x.data_ptr() for x in dsl], [r[2] for r in ranges])
    ref_parts = [(off, cnt, sp, sl) for (off, cnt, sp), sl in zip(ranges, slices)]
    return (p, g, m, v), dsl, args, ref_parts


@pytest.mark.parametrize("scale", ["tabular", "unit"])
@pytest.mark.parametrize("case", C.PARTS_CASES, ids=[c[0] for c in C.PARTS_CASES])
def test_adam_reads_split_k_partials_for_its_ranges_and_g_elsewhere(case, scale):
    """g over every part range and the slice slots past ``splits`` hold NaN: a read of the wrong source is non-finite,
    a wrong slice count or stride is out of bound."""
    nat, t = _nat(), 10
    cpu, dsl, args, ref_parts = _part_setup(case, scale)
    s = AdamState(*cpu)
    for hp in C.HYPERS:
        dref = _to_dev(C.adam_ref(*cpu, t, hp, parts=ref_parts, device_counter=True))
        for launcher in ("adam_flat_step_parts", "adam_range"):
            s.reset()
            _launch(nat, launcher, s, hp, t, _step_tensor(t), parts=args)
            s.check("%s %s %s" % (launcher, case[0], hp), dref)


def test_adam_range_updates_its_elements_only():
    nat, n, t, hp = _nat(), C.RANGE_N, 3, C.HYPERS[3]
    cpu = C.adam_inputs(n, "unit", seed=2)
    s = AdamState(*cpu)
    step = _step_tensor(t)
    got = {}
    for lo, hi in C.RANGES + [(0, n)]:
        dref = _to_dev(C.adam_ref(*cpu, t, hp, lo=lo, hi=hi, device_counter=True))
        s.reset()
        _launch(nat, "adam_range", s, hp, t, step, lo=lo, hi=hi)
        s.check("adam_range [%d, %d)" % (lo, hi), dref)
        out = (dref.p_bound == 0).nonzero().flatten()
        for x, x0 in zip((s.p, s.m, s.v), (s.init[0], s.init[2], s.init[3])):
            assert _same_bits(x[out], x0[out]), "elements outside [%d, %d) changed" % (lo, hi)
        got[(lo, hi)] = [x.clone() for x in (s.p, s.m, s.v, s.pb)]
    # two disjoint launches on one state = one full launch, bit for bit
    s.reset()
    for lo, hi in C.RANGES[:2]:
        _launch(nat, "adam_range", s, hp, t, step, lo=lo, hi=hi)
    for a, b in zip((s.p, s.m, s.v, s.pb), got[(0, n)]):
        assert _same_bits(a, b)
    assert int(step.item()) == t


@pytest.mark.parametrize("launcher", ["adam_flat_step", "adam_flat_step_parts", "adam_range", "step_end"])
def test_step_epilogue_records_the_loss_and_advances_the_cursor_once(launcher):
    """loss_out[*cursor] = *loss_slot inside [0, cap) only; cursor += 1 always, once per launch (600000 elements:
    586 workgroups)."""
    nat, cap, n, hp = _nat(), 5, 600000, C.HYPERS[0]
    s = AdamState(*C.adam_inputs(n, "unit", seed=3)) if launcher != "step_end" else None
    slot = torch.tensor([0.75], device=_dev())
    step = _step_tensor(4)
    for c0 in (-1, 0, cap - 1, cap):
        cur = torch.tensor([c0, GUARD_I32], dtype=torch.int32, device=_dev())
        out = torch.full((cap + 1,), float("nan"), device=_dev())
        if launcher == "step_end":
            nat.step_end(cur.data_ptr(), slot.data_ptr(), out.data_ptr(), cap, _st())
            torch.cuda.synchronize()
        else:
            s.reset()
            _launch(nat, launcher, s, hp, 4, step, cursor=cur.data_ptr(), slot=slot.data_ptr(), out=out.data_ptr(), cap=cap)
        assert cur.tolist() == [c0 + 1, GUARD_I32], (c0, cur.tolist())
        want = [0.75 if i == c0 and 0 <= c0 < cap else None for i in range(cap + 1)]
        got = [None if x != x else x for x in out.tolist()]
        assert got == want, (c0, got)
        assert float(slot.item()) == 0.75 and int(step.item()) == 4


def test_adam_launchers_refuse_bad_arguments_and_touch_nothing():
    nat, n, hp, t = _nat(), 4099, C.HYPERS[3], 3
    s = AdamState(*C.adam_inputs(n, "unit", seed=4))
    step = _step_tensor(t)
    part = torch.full((9, 512), 1.0, device=_dev())
    one = lambda off, cnt, sp, ptr=None: ([off], [cnt], [part.data_ptr() if ptr is None else ptr], [sp])  # noqa: E731
    p, g, m, v, pb = s.ptrs()
    bad = [
        ("lo % 4 != 0", "adam_range", dict(lo=2, hi=2048)),
        ("hi % 4 != 0 and hi != n", "adam_range", dict(lo=0, hi=1026)),
        ("empty range", "adam_range", dict(lo=1024, hi=1024)),
        ("part range past n & ~3", "adam_range", dict(parts=one(4096 - 508, 512, 2))),
        ("part range past n & ~3", "adam_flat_step_parts", dict(parts=one(4096 - 508, 512, 2))),
        ("part offset % 4 != 0", "adam_flat_step_parts", dict(parts=one(6, 512, 2))),
        ("splits = 9", "adam_range", dict(parts=one(0, 512, 9))),
        ("splits = 9", "adam_flat_step_parts", dict(parts=one(0, 512, 9))),
        ("splits = 0", "adam_flat_step_parts", dict(parts=one(0, 512, 0))),
        ("misaligned partials", "adam_flat_step_parts", dict(parts=one(0, 512, 2, part.data_ptr() + 4))),
        ("misaligned p", "adam_range", dict(n=n - 1, ptrs=(p + 4, g, m, v, pb))),
        ("misaligned g", "adam_flat_step_parts", dict(n=n - 1, ptrs=(p, g + 4, m, v, pb))),
        ("misaligned m", "adam_flat_step", dict(n=n - 1, ptrs=(p, g, m + 4, v, pb))),
        ("misaligned v", "adam_flat", dict(n=n - 1, ptrs=(p, g, m, v + 4, pb))),
        ("no step counter", "adam_range", dict(step=None)),
        ("no step counter", "adam_flat_step_parts", dict(step=None)),
    ]
    for what, launcher, kw in bad:
        kw = dict(kw)
        st = kw.pop("step", step)
        with pytest.raises(RuntimeError, match="invalid"):
            _launch(nat, launcher, s, hp, t, st, **kw)
        torch.cuda.synchronize()
        assert s.untouched(), what + " (%s): a refused launch changed a buffer" % launcher
    cur = torch.tensor([0], dtype=torch.int32, device=_dev())
    with pytest.raises(RuntimeError, match="invalid"):  # a cursor without a loss slot
        _launch(nat, "adam_flat_step", s, hp, t, step, cursor=cur.data_ptr())
    assert s.untouched() and int(cur.item()) == 0 and int(step.item()) == t


# ---------------------------------------------------------------------------------------------- (b) dW partials
@functools.lru_cache(maxsize=None)
def _dw_problem(M, N, K, splits):
    gen = torch.Generator().manual_seed(M + N + K)
    dz = (torch.randn(K, M, generator=gen) * 0.5).to(torch.bfloat16)
    x = (torch.randn(K, N, generator=gen) * 0.5).to(torch.bfloat16)
    refs = [C.gemm_ref(dz[k0:k1].T, x[k0:k1]) for k0, k1 in C.dw_slices(K, splits)]
    col0 = torch.randn(M, generator=gen).float()
    return dz, x, refs, col0


def _check_dw(what, M, N, K, splits, part, colsum):
    dz, x, refs, col0 = _dw_problem(M, N, K, splits)
    worst = 0.0
    for s, ((k0, k1), (ref, ab)) in enumerate(zip(C.dw_slices(K, splits), refs)):
        worst = max(worst, _ratio("%s slice %d k [%d, %d)" % (what, s, k0, k1), part[s * M * N:(s + 1) * M * N].cpu(),
                                  ref.reshape(-1), C.partial_bound(ref, ab, k1 - k0).reshape(-1)))
    assert float(part[splits * M * N]) == 123.0, what + ": wrote past the last slice"
    # column sums of dZ onto the initial colsum: K + 1 fp32 additions of terms that |colsum| + sum|dZ| bounds
    cs = col0.double() + dz.double().sum(0)
    cb = (K + 1) * C.U * (col0.double().abs() + dz.double().abs().sum(0)) * C.SECOND_ORDER
    rc = _ratio(what + " colsum", colsum[:M].cpu(), cs, cb)
    assert float(colsum[M]) == 123.0 and worst <= 1.0 and rc <= 1.0, (what, worst, rc)


def _dw_buffers(M, N, K, splits):
    dz, x, _, col0 = _dw_problem(M, N, K, splits)
    part = torch.full((splits * M * N + 1,), float("nan"), device=_dev())
    part[-1] = 123.0
    colsum = torch.cat([col0, torch.full((1,), 123.0)]).to(_dev())
    return dz.to(_dev()), x.to(_dev()), part, colsum


@pytest.mark.parametrize("rider", ["none", "scalar", "float4"])
@pytest.mark.parametrize("M,N,K,splits", [c[:4] for c in C.DW_CASES], ids=["x".join(map(str, c[:4])) for c in C.DW_CASES])
def test_dw_partials_match_fp64_slice_by_slice(M, N, K, splits, rider):
    """part[s] against the fp64 product over exactly slice s's k range, colsum against the fp64 column sums of dZ added
    onto a non-zero start - alone, and with an Adam range riding in the launch (which must come out right too)."""
    nat, t, hp = _nat(), 10, C.HYPERS[5]
    dz, x, part, colsum = _dw_buffers(M, N, K, splits)
    r = None
    if rider != "none":
        cpu, dsl, args, ref_parts = _part_setup(C.PARTS_CASES[1], "tabular")
        s = AdamState(*cpu)
        step = _step_tensor(t)
        r = nat.AdamRange(*s.ptrs(), s.n, *_hp_args(hp), hp.grad_scale, hp.decoupled, step.data_ptr(), *args, 0, s.n)
    nat.gemm_bf16_dw_partials_adam(dz.data_ptr(), x.data_ptr(), part.data_ptr(), colsum.data_ptr(), M, N, K, splits, r,
                                   1 if rider == "float4" else 0, _st())
    torch.cuda.synchronize()
    _check_dw("dW %dx%dx%d/%d %s" % (M, N, K, splits, rider), M, N, K, splits, part, colsum)
    if r is not None:
        s.check("riding Adam (%s)" % rider,
                _to_dev(C.adam_ref(*cpu, t, hp, parts=ref_parts, device_counter=True)))


@pytest.mark.parametrize("n,pcase,f4,kernel", C.RIDE_CASES, ids=[c[3].split(":")[0] + "-%d" % c[0] for c in C.RIDE_CASES])
def test_adam_riding_in_the_dw_launch_matches_fp64(n, pcase, f4, kernel):
    nat, t = _nat(), 2
    M, N, K, splits = C.DW_CASES[0][:4]
    dz, x, part, colsum = _dw_buffers(M, N, K, splits)
    if pcase:
        cpu, dsl, args, ref_parts = _part_setup({c[0]: c for c in C.PARTS_CASES}[pcase], "tabular")
    else:
        cpu, args, ref_parts = C.adam_inputs(n, "tabular", seed=6), ((), (), (), ()), None
    s = AdamState(*cpu)
    step = _step_tensor(t)
    for hp in C.HYPERS:
        s.reset()
        part[:-1] = float("nan")
        colsum.copy_(torch.cat([_dw_problem(M, N, K, splits)[3], torch.full((1,), 123.0)]))
        r = nat.AdamRange(*s.ptrs(), n, *_hp_args(hp), hp.grad_scale, hp.decoupled, step.data_ptr(), *args, 0, n)
        nat.gemm_bf16_dw_partials_adam(dz.data_ptr(), x.data_ptr(), part.data_ptr(), colsum.data_ptr(), M, N, K, splits,
                                       r, f4, _st())
        torch.cuda.synchronize()
        s.check("%s %s" % (kernel.split(":")[0], hp),
                _to_dev(C.adam_ref(*cpu, t, hp, parts=ref_parts, device_counter=True)))
        _check_dw("dW beside it", M, N, K, splits, part, colsum)
    assert int(step.item()) == t


def test_dw_partials_refuse_slices_without_a_k_tile():
    nat = _nat()
    for M, N, K, splits, what in C.DW_REJECTED:
        gen = torch.Generator().manual_seed(0)
        dz = torch.randn(K, M, generator=gen).to(torch.bfloat16).to(_dev())
        x = torch.randn(K, N, generator=gen).to(torch.bfloat16).to(_dev())
        part = torch.full((splits * M * N,), float("nan"), device=_dev())
        colsum = torch.full((M,), 2.0, device=_dev())
        s = AdamState(*C.adam_inputs(1037, "unit", seed=7))
        step = _step_tensor(3)
        hp = C.HYPERS[0]
        r = nat.AdamRange(*s.ptrs(), s.n, *_hp_args(hp), hp.grad_scale, hp.decoupled, step.data_ptr(), [], [], [], [], 0, s.n)
        for rr in (None, r):
            with pytest.raises(RuntimeError, match="invalid"):
                nat.gemm_bf16_dw_partials_adam(dz.data_ptr(), x.data_ptr(), part.data_ptr(), colsum.data_ptr(), M, N, K,
                                               splits, rr, 0, _st())
            torch.cuda.synchronize()
            assert bool(torch.isnan(part).all()) and bool((colsum == 2.0).all()) and s.untouched(), what
    # a bad Adam range refuses the whole launch, GEMM included
    M, N, K, splits = C.DW_CASES[2][:4]
    dz, x, part, colsum = _dw_buffers(M, N, K, splits)
    before = colsum.clone()
    r = nat.AdamRange(*s.ptrs(), s.n, *_hp_args(hp), hp.grad_scale, hp.decoupled, step.data_ptr(), [], [], [], [], 2, s.n)
    with pytest.raises(RuntimeError, match="invalid"):
        nat.gemm_bf16_dw_partials_adam(dz.data_ptr(), x.data_ptr(), part.data_ptr(), colsum.data_ptr(), M, N, K, splits,
                                       r, 0, _st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(part[:-1]).all()) and _same_bits(colsum, before) and s.untouched()


# ---------------------------------------------------------------------------------------------- (c) gathered forward
@functools.lru_cache(maxsize=None)
def _gather_problem(M, N, K):
    """Inputs on the device and the fp64 pre-activation of EVERY dataset row (computed once; each case gathers its
    rows from it)."""
    X, W, bias, Y, idxs = C.gather_inputs(M, N, K, seed=M + N + K)
    prod, ab = C.gemm_ref(X[:, :K], W.T)
    d = _dev()
    return dict(Xpad=X.to(d), Xtight=X[:, :K].contiguous().to(d), W=W.to(d), bias=bias.to(d), Y=Y.to(d),
                idx={k: v.to(d) for k, v in idxs.items()}, idx_cpu=idxs, z=(prod + bias.double()).to(d), ab=ab.to(d))


def _gather_launch(nat, pr, M, N, K, epi, ldx, idx, cursor, zoff=None, zcnt=None, C_=None):
    stride, n_items, n_idx, _ = C.batch_geometry(M)
    d = _dev()
    bufs = dict(
        C=torch.full((M + 1, N), GUARD_BF16, dtype=torch.bfloat16, device=d),
        aux=torch.full((M + 1, N), GUARD_BF16, dtype=torch.bfloat16, device=d),
        # the guard after a_out's M x K rows also holds a write with the dataset's row stride instead of K
        a_out=torch.full((M * (K + C.LDX_PAD) + K,), GUARD_BF16, dtype=torch.bfloat16, device=d),
        ydst=torch.full((M + 1,), GUARD_I32, dtype=torch.int32, device=d),
        step=torch.tensor([41, GUARD_I32], dtype=torch.int32, device=d),
        zero=torch.full((C.ZERO_LEN,), float("nan"), device=d),
        cursor=torch.tensor([cursor], dtype=torch.int32, device=d),
    )
    X = pr["Xpad"] if ldx != K else pr["Xtight"]
    zoff = [o for o, _ in C.ZERO_RANGES] if zoff is None else zoff
    zcnt = [c for _, c in C.ZERO_RANGES] if zcnt is None else zcnt
    nat.gemm_bf16_gather_fwd(X.data_ptr(), ldx, pr["W"].data_ptr(), bufs["C"].data_ptr(), pr["bias"].data_ptr(), M, N, K,
                             epi, bufs["aux"].data_ptr() if epi == C.EPI_BIAS_GELU else 0, pr["idx"][idx].data_ptr(),
                             bufs["cursor"].data_ptr(), stride, n_items, bufs["a_out"].data_ptr(), pr["Y"].data_ptr(),
                             bufs["ydst"].data_ptr(), bufs["step"].data_ptr(), bufs["zero"].data_ptr(), zoff, zcnt, _st())
    torch.cuda.synchronize()
    return bufs


EPIS = [(C.EPI_BIAS, "bias"), (C.EPI_BIAS_RELU, "bias_relu"), (C.EPI_BIAS_GELU, "bias_gelu_aux")]


@pytest.mark.parametrize("epi,epi_name", EPIS, ids=[e[1] for e in EPIS])
@pytest.mark.parametrize("M,N,K,kernel", [c[:4] for c in C.GATHER_CASES],
                         ids=["x".join(map(str, c[:3])) for c in C.GATHER_CASES])
def test_gathered_forward_gemm_and_its_side_effects(M, N, K, kernel, epi, epi_name):
    """Tight and padded dataset rows x a permutation and repeated rows x a batch inside the list and one whose second
    half wraps: C (and GELU's aux) inside the bf16 bound of the fp64 product of the gathered rows; a_out, the
    labels, the step counter and the cleared ranges exact; nothing written past any of them."""
    nat = _nat()
    cus = nat.device_cu_count()
    reached = C.gather_kernel(M, N, K, cus)
    print("  %d compute units: %s" % (cus, reached))
    if reached != kernel:
        pytest.skip("%d compute units: %dx%dx%d reaches %s, not the %s this case is for" % (cus, M, N, K, reached, kernel))
    pr = _gather_problem(M, N, K)
    stride, n_items, n_idx, cursors = C.batch_geometry(M)
    zmask = C.zero_mask().to(_dev())
    for ldx in (K, K + C.LDX_PAD):
        for idx in ("permutation", "repeated"):
            for cursor in cursors:
                what = "%s ldx=%d %s cursor=%d" % (epi_name, ldx, idx, cursor)
                rows = C.gather_rows_ref(pr["idx_cpu"][idx], cursor, stride, n_items, M).to(_dev())
                b = _gather_launch(nat, pr, M, N, K, epi, ldx, idx, cursor)
                z, ab = pr["z"][rows], pr["ab"][rows]
                if epi == C.EPI_BIAS:
                    rc = _ratio(what + " C", b["C"][:M], z, C.fwd_bound(z, ab, K))
                elif epi == C.EPI_BIAS_RELU:
                    rc = _ratio(what + " C", b["C"][:M], z.clamp_min(0), C.fwd_bound(z, ab, K))
                else:
                    rc = _ratio(what + " C", b["C"][:M], C.gelu_ref(z), C.gelu_out_bound(z, ab, K))
                    ra = _ratio(what + " aux", b["aux"][:M], z, C.fwd_bound(z, ab, K))
                    assert ra <= 1.0, (what, ra)
                assert rc <= 1.0, (what, rc)
                assert _same_bits(b["a_out"][:M * K].view(M, K), pr["Xtight"][rows]), what + ": a_out != X[rows, :K]"
                assert bool((b["a_out"][M * K:] == GUARD_BF16).all()), what + ": wrote past a_out"
                assert torch.equal(b["ydst"][:M], pr["Y"][rows]), what + ": labels"
                assert int(b["ydst"][M]) == GUARD_I32 and b["step"].tolist() == [42, GUARD_I32], what
                assert int(b["cursor"].item()) == cursor
                assert bool((b["zero"][zmask] == 0).all()) and bool(torch.isnan(b["zero"][~zmask]).all()), what + ": zero ranges"
                assert bool((b["C"][M] == GUARD_BF16).all()), what + ": wrote past C"
                if epi == C.EPI_BIAS_GELU:
                    assert bool((b["aux"][M] == GUARD_BF16).all()), what + ": wrote past aux"
                else:
                    assert bool((b["aux"] == GUARD_BF16).all()), what + ": aux written without GELU"


def test_gathered_forward_refuses_shapes_and_epilogues_it_has_no_kernel_for():
    nat = _nat()
    for M, N, K, epi, nz, what in C.GATHER_REJECTED:
        gen = torch.Generator().manual_seed(1)
        d = _dev()
        rows = 3 * M + 7
        pr = dict(Xtight=torch.randn(rows, K, generator=gen).to(torch.bfloat16).to(d),
                  W=torch.randn(N, K, generator=gen).to(torch.bfloat16).to(d), bias=torch.zeros(N, device=d),
                  Y=torch.zeros(rows, dtype=torch.int32, device=d),
                  idx={"permutation": torch.arange(3 * M, dtype=torch.int32, device=d)})
        pr["Xpad"] = pr["Xtight"]
        zoff, zcnt = [0, 8, 16, 24, 32][:nz], [4] * nz
        with pytest.raises(RuntimeError, match="invalid"):
            _gather_launch(nat, pr, M, N, K, epi, K, "permutation", 0, zoff, zcnt)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- (d) step kernels
def _batch_problem(B, rb, wide):
    gen = torch.Generator().manual_seed(B + rb)
    stride, n_items, n_idx, cursors = C.batch_geometry(B)
    rows = n_idx + 7
    it = torch.int64 if wide else torch.int32
    X = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, rb // 4), generator=gen, dtype=torch.int64).to(torch.int32)
    Y = torch.randint(0, 1 << 20, (rows,), generator=gen).to(it)
    idx = torch.randperm(rows, generator=gen)[:n_idx].to(it)
    return X, Y, idx, stride, n_items, cursors


def _batch_buffers(B, rb, wide):
    d = _dev()
    return dict(x=torch.full((B + 1, rb // 4), GUARD_I32, dtype=torch.int32, device=d),
                y=torch.full((B + 1,), GUARD_I32, dtype=torch.int64 if wide else torch.int32, device=d),
                step=torch.tensor([41, GUARD_I32], dtype=torch.int32, device=d),
                zero=torch.full((C.ZERO_LEN,), float("nan"), device=d))


def _check_batch(what, b, B, X, Y, rows, stepped):
    assert torch.equal(b["x"][:B].cpu(), X[rows]), what + ": rows"
    assert torch.equal(b["y"][:B].cpu(), Y[rows]), what + ": labels"
    assert bool((b["x"][B] == GUARD_I32).all()) and int(b["y"][B]) == GUARD_I32, what + ": wrote past the batch"
    assert b["step"].tolist() == [41 + stepped, GUARD_I32], what + ": step counter"


@pytest.mark.parametrize("B,rb", C.STEP_CASES)
def test_batch_gather_with_the_step_prologue_riding_along(B, rb):
    """dct_gather_batch_step_ranges against gather_rows_ref, exactly: a batch inside the item list and one whose second
    half wraps; the step counter + 1 once (also where the zero range, not the batch, sizes the grid); the four zero
    ranges.  Without counter and ranges it is dct_gather_batch."""
    nat = _nat()
    X, Y, idx, stride, n_items, cursors = _batch_problem(B, rb, False)
    dX, dY, didx = X.to(_dev()), Y.to(_dev()), idx.to(_dev())
    zmask = C.zero_mask().to(_dev())
    for cursor in cursors:
        rows = C.gather_rows_ref(idx, cursor, stride, n_items, B)
        cur = torch.tensor([cursor], dtype=torch.int32, device=_dev())
        for ride in (True, False):
            b = _batch_buffers(B, rb, False)
            nat.gather_batch_step_ranges(dX.data_ptr(), rb, dY.data_ptr(), didx.data_ptr(), cur.data_ptr(), stride, B,
                                         n_items, b["x"].data_ptr(), b["y"].data_ptr(),
                                         b["step"].data_ptr() if ride else 0, b["zero"].data_ptr() if ride else 0,
                                         [o for o, _ in C.ZERO_RANGES] if ride else [],
                                         [c for _, c in C.ZERO_RANGES] if ride else [], _st())
            torch.cuda.synchronize()
            _check_batch("B=%d rb=%d cursor=%d ride=%s" % (B, rb, cursor, ride), b, B, X, Y, rows, int(ride))
            if ride:
                assert bool((b["zero"][zmask] == 0).all()) and bool(torch.isnan(b["zero"][~zmask]).all())
            else:
                assert bool(torch.isnan(b["zero"]).all())
            assert int(cur.item()) == cursor
    # B = 0: nothing launched, nothing touched; five ranges: refused
    b = _batch_buffers(B, rb, False)
    nat.gather_batch_step_ranges(dX.data_ptr(), rb, dY.data_ptr(), didx.data_ptr(), cur.data_ptr(), stride, 0, n_items,
                                 b["x"].data_ptr(), b["y"].data_ptr(), b["step"].data_ptr(), b["zero"].data_ptr(),
                                 [0], [8], _st())
    with pytest.raises(RuntimeError, match="invalid"):
        nat.gather_batch_step_ranges(dX.data_ptr(), rb, dY.data_ptr(), didx.data_ptr(), cur.data_ptr(), stride, B,
                                     n_items, b["x"].data_ptr(), b["y"].data_ptr(), b["step"].data_ptr(),
                                     b["zero"].data_ptr(), [0, 8, 16, 24, 32], [4] * 5, _st())
    torch.cuda.synchronize()
    assert bool((b["x"] == GUARD_I32).all()) and bool((b["y"] == GUARD_I32).all()) and b["step"].tolist() == [41, GUARD_I32]
    assert bool(torch.isnan(b["zero"]).all())


@pytest.mark.parametrize("B,rb", C.STEP_CASES)
def test_autograd_step_prologue(B, rb):
    """dct_ag_step_prologue (int64 labels and indices, stride = B, one zero range [0, zero_n))."""
    nat = _nat()
    X, Y, idx, stride, n_items, cursors = _batch_problem(B, rb, True)
    dX, dY, didx = X.to(_dev()), Y.to(_dev()), idx.to(_dev())
    for cursor, zero_n in zip(cursors, (7, 1030)):
        rows = C.gather_rows_ref(idx, cursor, B, n_items, B)
        cur = torch.tensor([cursor], dtype=torch.int32, device=_dev())
        b = _batch_buffers(B, rb, True)
        nat.ag_step_prologue(dX.data_ptr(), rb, dY.data_ptr(), didx.data_ptr(), cur.data_ptr(), B, n_items,
                             b["x"].data_ptr(), b["y"].data_ptr(), b["step"].data_ptr(), b["zero"].data_ptr(), zero_n, _st())
        torch.cuda.synchronize()
        _check_batch("ag B=%d rb=%d cursor=%d" % (B, rb, cursor), b, B, X, Y, rows, 1)
        assert bool((b["zero"][:zero_n] == 0).all()) and bool(torch.isnan(b["zero"][zero_n:]).all())
        assert int(cur.item()) == cursor


@pytest.mark.parametrize("n", C.ZERO_NS)
def test_zero_f32_clears_n_values_and_no_more(n):
    nat = _nat()
    buf = torch.full((n + 5,), float("nan"), device=_dev())
    nat.zero_f32(buf.data_ptr(), n, _st())
    torch.cuda.synchronize()
    assert bool((buf[:n] == 0).all()) and bool(torch.isnan(buf[n:]).all())
    with pytest.raises(RuntimeError, match="invalid"):
        nat.zero_f32(buf.data_ptr() + 4, 1, _st())
