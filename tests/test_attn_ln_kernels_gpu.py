"""The per-op attention, LayerNorm and gather kernels, each launcher on its own, element by element against the fp64
references and derived bounds of tests/attn_ln_cases.py: every instantiation of attn_fwd_mfma / attn_bwd_mfma with one,
five and six live waves, the scalar attention kernels at every T and D the launcher takes (a second pass of the thread
loops, the 128 KB forward, padded and odd row strides), MFMA-shaped calls that must fall back, every narrow and the
generic LayerNorm kernel in every dtype / operand combination (idle lanes, second grid-stride passes, shared slot rows,
the workspace re-zeroed), both gather kernels, and every refusal.  One launch per case; every output lands in a
guard-filled buffer with a guard region after it (and before it, where the buffer starts off alignment); every
comparison is kernel against reference on the CPU; every test prints its worst error / bound ratio per tensor before it
asserts <= 1.  The backward of attention is evaluated on the kernel's own bf16 o and fp32 lse of the forward launch.

Measured on an MI355X (2026-10-21): worst error / bound per tensor over every case of a path; "unit / edge" input sets.

  attention, MFMA path (all twelve instantiations, 1 / 5 / 6 live waves, padded strides):
    o 0.758 / 0.868   lse 0.114 / 0.074   dq 0.671 / 0.844   dk 0.702 / 0.872   dv 0.667 / 0.919
  attention, scalar path (T = 1 .. 512, D = 1 .. 64):
    o 0.985 / 0.968   lse 0.103 / 0.209   dq 0.977 / 0.965   dk 0.991 / 0.985   dv 0.988 / 0.984
  attention, MFMA-shaped calls held to the scalar bound (q / k / v, the stride, o or dout off alignment):
    o 0.981 / 0.943 (0.560 / 0.691 where only o or dout is off: that forward is the MFMA kernel under its own bound)
    lse 0.059 / 0.057   dq 0.963 / 0.964   dk 0.987 / 0.959   dv 0.984 / 0.974
  layernorm_fwd_small<LPR>: y 0.197 / 0.212 (bf16 out 0.995 / 0.992)   mean 0.208 / 0.218   rstd 0.235 / 0.366
  layernorm_fwd_kernel:     y 0.209 / 0.255 (bf16 out 0.988 / 0.991)   mean 0.279 / 0.328   rstd 0.368 / 0.368
    (w or b one float into a buffer: y 0.042, rstd 0.251, bf16 y 0.991 - the generic kernel's figures at N = 64)
  layernorm_bwd_small<LPR> + fold, all 32 operand combinations:
                                   fp32 dx 0.470 / 0.869   bf16 dx 0.994 / 0.995   dw 0.113 / 0.101   db 0.067 / 0.094
  layernorm_bwd_kernel:            fp32 dx 0.349 / 0.425   bf16 dx 0.993 / 0.994   dw 0.316 / 0.283   db 0.238 / 0.297
  gather: every case bit-equal

Above 0.9 only by their own final bf16 rounding, and nothing to watch: the scalar attention path's o, dq, dk, dv (P and
dS stay fp32 there, so the bound is 2^-8 |value| plus accumulation terms a hundred times smaller; the worst element sits
next to a rounding tie), every bf16 y and bf16 dx.  The torch emulations of tests/test_attn_ln_cases_cpu.py give the
same figures (scalar 0.92 - 0.99, MFMA 0.42 - 0.91, whose bound carries the hidden bf16 roundings of P and dS).  The
fp32 outputs stay below 0.48, but for the narrow backward's fp32 dx on the edge set (0.805 and 0.869 at N = 4 and 8,
falling to 0.153 at N = 256: at the narrowest rows the bound is a handful of roundings with little slack); lse stays
below 0.21.

No kernel was found wrong.  Three launcher conditions were, by reading, and are fixed on the host side: attn_mfma did
not look at o's alignment before the MFMA backward's 8-byte loads of it; dct_layernorm_fwd did not look at b's, nor
dct_layernorm_bwd_ex at w's, before the narrow kernels' float4 loads.  The cases that hand those launchers such a
pointer were first run after the fix.
"""
import functools

import pytest
import torch

import attn_ln_cases as C

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = {torch.float32: -7.25, torch.bfloat16: -7.0, torch.uint8: 0xA5}
PADV = 7.0  # what the padding of an INPUT row holds: finite, and wrong wherever it were read as data
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8


def _nat():
    from dct_amd.ops._native import native

    return native()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev():
    return torch.device("cuda", 0)


class Buf:
    """An output buffer of n elements starting ``shift`` elements into a 16-byte aligned allocation, guard-filled,
    with GUARD more elements after it (and the ``shift`` before it)."""

    def __init__(self, n, dtype, init=None, shift=0):
        self.n, self.shift, self.fill = n, shift, FILL[dtype]
        self.all = torch.full((shift + n + GUARD,), self.fill, dtype=dtype, device=_dev())
        assert self.all.data_ptr() % 16 == 0
        self.t = self.all[shift:shift + n]
        if init is not None:
            self.t.copy_(init.reshape(-1).to(_dev()))

    @property
    def ptr(self):
        return self.all.data_ptr() + self.shift * self.all.element_size()

    def guard_ok(self):
        before, after = self.all[:self.shift], self.all[self.shift + self.n:]
        return bool((before == self.fill).all()) and bool((after == self.fill).all())

    def untouched(self):
        return bool((self.all == self.fill).all())

    def cpu(self, *shape):
        return self.t.cpu().reshape(*shape) if shape else self.t.cpu()


class In:
    """An input on the device, ``shift`` elements into a 16-byte aligned allocation."""

    def __init__(self, t, shift=0):
        self.all = torch.zeros(shift + t.numel() + 8, dtype=t.dtype, device=_dev())
        assert self.all.data_ptr() % 16 == 0
        self.all[shift:shift + t.numel()].copy_(t.reshape(-1).to(_dev()))
        self.ptr = self.all.data_ptr() + shift * self.all.element_size()


def _worst(what, ratios):
    print("  %s: %s" % (what, "  ".join("%s %.3f" % (k, v) for k, v in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (what, bad)


def _merge(worst, r, prefix=""):
    for k, v in r.items():
        worst[prefix + k] = max(worst.get(prefix + k, 0.0), v)


def _refused(fn, *args):
    with pytest.raises(RuntimeError):
        fn(*args)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- attention
def _pack(parts, ld):
    """[M][ld] bf16 rows: the parts' rows side by side, PADV in the padding."""
    M = parts[0].shape[0]
    out = torch.full((M, ld), PADV, dtype=BF16)
    col = 0
    for p in parts:
        out[:, col:col + p.shape[1]] = p
        col += p.shape[1]
    return out


def _att_launch(c, kind):
    """One forward and (unless fwd_only) one backward launch of the case; {tensor: ratio}."""
    nat = _nat()
    T, D, Bsz, H = c["T"], c["D"], c["Bsz"], c["H"]
    HD, M, (ldq, ldo), sh = H * D, Bsz * T, C.att_ld(c), c["shift"]
    q, k, v, do = C.att_inputs(c, kind)
    scale = C.f32scale(D)
    qkv = In(_pack([C.rows(q), C.rows(k), C.rows(v)], ldq), sh.get("qkv", 0))
    o, lse = Buf(M * ldo, BF16, shift=sh.get("o", 0)), Buf(Bsz * H * T, F32)
    nat.attention_fwd(qkv.ptr, qkv.ptr + 2 * HD, qkv.ptr + 4 * HD, o.ptr, lse.ptr, Bsz, H, T, D, ldq, ldo, scale, _st())
    torch.cuda.synchronize()
    what = C.att_name(c)
    assert o.guard_ok() and lse.guard_ok(), what
    orows = o.cpu(M, ldo)
    assert bool((orows[:, HD:] == o.fill).all()), "%s: o's padding written" % what
    got = {"o": C.from_rows(orows[:, :HD], Bsz, H), "lse": lse.cpu(Bsz, H, T)}
    r = C.attn_fwd_check(got, q, k, v, scale, C.is_mfma(C.attn_kernel(c, False)))
    if c["fwd_only"]:
        return r
    dqkv = Buf(M * ldq, BF16, shift=sh.get("qkv", 0))
    dout = In(_pack([C.rows(do)], ldo), sh.get("do", 0))
    nat.attention_bwd(qkv.ptr, qkv.ptr + 2 * HD, qkv.ptr + 4 * HD, o.ptr, dout.ptr, lse.ptr, dqkv.ptr,
                      dqkv.ptr + 2 * HD, dqkv.ptr + 4 * HD, Bsz, H, T, D, ldq, ldo, scale, _st())
    torch.cuda.synchronize()
    assert dqkv.guard_ok(), what
    drows = dqkv.cpu(M, ldq)
    assert bool((drows[:, 3 * HD:] == dqkv.fill).all()), "%s: dq / dk / dv's padding written" % what
    assert C.same_bits(o.cpu(M, ldo), orows) and C.same_bits(lse.cpu(Bsz, H, T), got["lse"]), what  # inputs here
    gb = {n: C.from_rows(drows[:, i * HD:(i + 1) * HD], Bsz, H) for i, n in enumerate(("dq", "dk", "dv"))}
    r.update(C.attn_bwd_check(gb, q, k, v, got["o"], got["lse"], do, scale, C.is_mfma(C.attn_kernel(c, True))))
    return r


MFMA_TD = [(T, D) for T in (16, 32, 48, 64) for D in (16, 32, 64)]


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("T,D", MFMA_TD)
def test_attention_mfma_instantiations(T, D, kind):
    """attn_fwd_mfma / attn_bwd_mfma<T / 16, D / 16> with (Bsz, H) = (1, 1): three dead waves; (2, 3): a dead half
    block; (5, 1); and the padded strides where the table has them."""
    cases = [c for c in C.ATT_MFMA if (c["T"], c["D"]) == (T, D)]
    assert len(cases) >= 3
    for c in cases:
        assert C.attn_kernel(c, False) == "attn_fwd_mfma<%d, %d>" % (T // 16, D // 16)
        _worst("%s %s" % (C.att_name(c), kind), _att_launch(c, kind))


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("c", C.ATT_SCALAR, ids=C.att_name)
def test_attention_scalar_kernels(c, kind):
    assert C.attn_kernel(c, False) == "attn_fwd_kernel"
    _worst("%s %s" % (C.att_name(c), kind), _att_launch(c, kind))


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("c", C.ATT_FALLBACK, ids=C.att_name)
def test_attention_mfma_shaped_calls_fall_back_to_the_scalar_kernels(c, kind):
    """Held to the bound of the kernel attn_kernel names: the scalar path's tighter one wherever a pointer or stride
    rules the 8-byte loads out (q / k / v, the row stride, dout - and o, which attn_mfma used not to look at)."""
    assert C.attn_kernel(c, True) == "attn_bwd_kernel"
    _worst("%s %s" % (C.att_name(c), kind), _att_launch(c, kind))


def test_attention_refusals_write_nothing():
    nat = _nat()
    both = dict(C.ATT_REFUSED)
    for name, c in list(both.items()) + list(C.ATT_REFUSED_BWD_ONLY.items()):
        T, D, Bsz, H = c["T"], c["D"], c["Bsz"], c["H"]
        HD, M, (ldq, ldo) = H * D, Bsz * max(T, 1), C.att_ld(c)
        scale = C.f32scale(D)
        qkv = In(torch.randn(M, ldq).to(BF16))
        dout = In(torch.randn(M, ldo).to(BF16))
        o, lse, dqkv = Buf(M * ldo, BF16), Buf(Bsz * H * max(T, 1), F32), Buf(M * ldq, BF16)
        if name in both:
            assert C.attn_kernel(c, False) == "refused"
            _refused(nat.attention_fwd, qkv.ptr, qkv.ptr + 2 * HD, qkv.ptr + 4 * HD, o.ptr, lse.ptr, Bsz, H, T, D, ldq,
                     ldo, scale, _st())
        oin, lin = In(torch.randn(M, ldo).to(BF16)), In(torch.randn(Bsz * H * max(T, 1)))
        assert C.attn_kernel(c, True) == "refused"
        _refused(nat.attention_bwd, qkv.ptr, qkv.ptr + 2 * HD, qkv.ptr + 4 * HD, oin.ptr, dout.ptr, lin.ptr, dqkv.ptr,
                 dqkv.ptr + 2 * HD, dqkv.ptr + 4 * HD, Bsz, H, T, D, ldq, ldo, scale, _st())
        assert o.untouched() and lse.untouched() and dqkv.untouched(), name
        print("  refused: %s" % name)


# ---------------------------------------------------------------------------------------------- LayerNorm forward
def _ln_fwd_launch(M, N, kind, in_bf16, out_bf16, nulls="", shift=()):
    """One dct_layernorm_fwd launch; ``nulls``: operands passed as null; ``shift``: operands one float into their
    buffer.  Returns {tensor: ratio}."""
    nat = _nat()
    i = C.ln_inputs(M, N, kind, in_bf16)
    w, b = (None if "w" in nulls else i["w"]), (None if "b" in nulls else i["b"])
    x = In(i["x"])
    wd = In(w, 1 if "w" in shift else 0) if w is not None else None
    bd = In(b, 1 if "b" in shift else 0) if b is not None else None
    y, mean, rstd = Buf(M * N, BF16 if out_bf16 else F32), Buf(M, F32), Buf(M, F32)
    stats = "stats" not in nulls
    nat.layernorm_fwd(x.ptr, wd.ptr if wd else 0, bd.ptr if bd else 0, y.ptr, mean.ptr if stats else 0,
                      rstd.ptr if stats else 0, M, N, C.EPS, in_bf16, out_bf16, _st())
    torch.cuda.synchronize()
    what = "ln fwd M=%d N=%d %s" % (M, N, nulls)
    assert y.guard_ok() and mean.guard_ok() and rstd.guard_ok(), what
    got = {"y": y.cpu(M, N)}
    if stats:
        got.update(mean=mean.cpu(), rstd=rstd.cpu())
    else:
        assert mean.untouched() and rstd.untouched(), what
    return C.ln_fwd_check(got, i["x"], w, b, out_bf16)


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("N", C.LN_FWD_NS)
def test_layernorm_forward(N, kind):
    worst = {}
    for M in C.LN_MS:
        for in_bf16, out_bf16 in C.LN_FWD_DTYPES:
            _merge(worst, _ln_fwd_launch(M, N, kind, in_bf16, out_bf16), "bf16 " if out_bf16 else "f32 ")
            if (M, N) in ((37, 64), (37, 260)):
                for nulls in C.LN_FWD_NULLS:
                    _merge(worst, _ln_fwd_launch(M, N, kind, in_bf16, out_bf16, nulls), "bf16 " if out_bf16 else "f32 ")
    _worst("%s N=%d %s" % (C.ln_fwd_kernel(37, N), N, kind), worst)


@pytest.mark.parametrize("kind", C.INPUT_SETS)
def test_layernorm_forward_second_grid_stride_pass(kind):
    M, N = C.LN_FWD_BIG
    assert C.ln_fwd_passes(M, N) == 2
    worst = {}
    for in_bf16, out_bf16 in ((0, 0), (1, 1)):
        _merge(worst, _ln_fwd_launch(M, N, kind, in_bf16, out_bf16), "bf16 " if out_bf16 else "f32 ")
    _worst("%s M=%d N=%d %s" % (C.ln_fwd_kernel(M, N), M, N, kind), worst)


@pytest.mark.parametrize("N,shift", [(64, "b"), (64, "w"), (1000, "w")])
def test_layernorm_forward_takes_the_generic_kernel_for_a_misaligned_w_or_b(N, shift):
    """w or b a view one float into a buffer (a flat parameter buffer does that): the narrow kernels' float4 loads
    cannot take it, and dct_layernorm_fwd now looks at b as well as w."""
    assert C.ln_fwd_kernel(37, N, aligned=False) == "layernorm_fwd_kernel"
    worst = {}
    for kind in C.INPUT_SETS:
        for in_bf16, out_bf16 in ((0, 0), (1, 1)):
            _merge(worst, _ln_fwd_launch(37, N, kind, in_bf16, out_bf16, shift=(shift,)),
                   "bf16 " if out_bf16 else "f32 ")
    _worst("layernorm_fwd_kernel N=%d %s one float in" % (N, shift), worst)


def test_layernorm_forward_refuses_n_2049():
    nat = _nat()
    M, N = 3, 2049
    assert C.ln_fwd_kernel(M, N) == "refused"
    x, w, b = In(torch.randn(M, N)), In(torch.randn(N)), In(torch.randn(N))
    y, mean, rstd = Buf(M * N, F32), Buf(M, F32), Buf(M, F32)
    _refused(nat.layernorm_fwd, x.ptr, w.ptr, b.ptr, y.ptr, mean.ptr, rstd.ptr, M, N, C.EPS, 0, 0, _st())
    assert y.untouched() and mean.untouched() and rstd.untouched()
    dx, dw, db = Buf(M * N, F32), Buf(N, F32), Buf(N, F32)
    _refused(nat.layernorm_bwd, x.ptr, x.ptr, w.ptr, mean.ptr, rstd.ptr, dx.ptr, dw.ptr, db.ptr, M, N, 0, _st())
    assert dx.untouched() and dw.untouched() and db.untouched()


# ---------------------------------------------------------------------------------------------- LayerNorm backward
@functools.lru_cache(maxsize=8)
def _ln_saved(M, N, kind, x_bf16):
    """mean / rstd as a forward saves them: any fp32 values are exact inputs of the backward (the CPU emulation's)."""
    i = C.ln_inputs(M, N, kind, x_bf16)
    g = C.emulate_ln_fwd(i["x"], i["w"], i["b"], 0)
    return g["mean"], g["rstd"]


class _LnBwdEx:
    """The operands of one dct_layernorm_bwd_ex problem on the device; launch() may be repeated on the same
    workspace."""

    def __init__(self, M, N, kind, mode, ws_zeroed=True):
        self.M, self.N, self.mode = M, N, mode
        dy_bf16, x_bf16, dx_bf16, dx2, dres = mode
        self.i = i = C.ln_inputs(M, N, kind, x_bf16, dy_bf16)
        self.mean, self.rstd = _ln_saved(M, N, kind, x_bf16)
        self.dy, self.x, self.md, self.rd = In(i["dy"]), In(i["x"]), In(self.mean), In(self.rstd)
        self.w = In(i["w"])
        self.dres = In(i["dres"]) if dres else None
        n_ws = _nat().layernorm_bwd_ws_floats(N)
        self.ws = Buf(n_ws, F32, init=torch.zeros(n_ws) if ws_zeroed else None)

    def launch(self, grads="wb"):
        M, N = self.M, self.N
        dy_bf16, x_bf16, dx_bf16, dx2, dres = self.mode
        out = dict(dx=Buf(M * N, BF16 if dx_bf16 else F32), dx2=Buf(M * N, BF16),
                   dw=Buf(N, F32, init=self.i["dw0"]), db=Buf(N, F32, init=self.i["db0"]))
        _nat().layernorm_bwd_ex(self.dy.ptr, dy_bf16, self.x.ptr, x_bf16, self.w.ptr, self.md.ptr, self.rd.ptr,
                                out["dx"].ptr, dx_bf16, out["dx2"].ptr if dx2 else 0,
                                self.dres.ptr if self.dres else 0, out["dw"].ptr if "w" in grads else 0,
                                out["db"].ptr if "b" in grads else 0, self.ws.ptr, M, N, _st())
        torch.cuda.synchronize()
        return out

    def check(self, out, grads, what):
        M, N, i = self.M, self.N, self.i
        dy_bf16, x_bf16, dx_bf16, dx2, dres = self.mode
        assert all(b.guard_ok() for b in out.values()) and self.ws.guard_ok(), what
        got = {"dx": out["dx"].cpu(M, N), "dw": out["dw"].cpu() if "w" in grads else None,
               "db": out["db"].cpu() if "b" in grads else None}
        if "w" not in grads:
            assert C.same_bits(out["dw"].cpu(), i["dw0"]), what + ": dw written"
        if "b" not in grads:
            assert C.same_bits(out["db"].cpu(), i["db0"]), what + ": db written"
        if dx2:  # the bf16 copy is the rounding of the same fp32 value
            assert C.same_bits(out["dx2"].cpu(M, N), C.bf(got["dx"])), what + ": dx2 is not bf16(dx)"
        else:
            assert out["dx2"].untouched(), what
        return C.ln_bwd_check(got, i["dy"], i["x"], i["w"], self.mean, self.rstd, i["dres"] if dres else None,
                              i["dw0"], i["db0"], C.ln_bwd_adders(M, N, True), dx_bf16)


def _ln_bwd_ex_cases(M, N, kind, modes, worst):
    for mode in modes:
        p = _LnBwdEx(M, N, kind, mode)
        what = "bwd_ex M=%d N=%d %s %s" % (M, N, kind, mode)
        out = p.launch("wb")
        _merge(worst, p.check(out, "wb", what), "bf16 " if mode[2] else "f32 ")
        assert bool((p.ws.t == 0).all()), what + ": workspace not re-zeroed"
        if mode is modes[0]:
            # again on the same workspace: the same bits in dx, dw / db within the bound again
            again = p.launch("wb")
            assert C.same_bits(again["dx"].cpu(), out["dx"].cpu()), what
            _merge(worst, p.check(again, "wb", what + " again"), "bf16 " if mode[2] else "f32 ")
            assert bool((p.ws.t == 0).all()), what
            for grads in ("w", "b"):
                one = p.launch(grads)
                assert C.same_bits(one["dx"].cpu(), out["dx"].cpu()), what
                _merge(worst, p.check(one, grads, what + " only d" + grads), "bf16 " if mode[2] else "f32 ")
                assert bool((p.ws.t == 0).all()), what
            # neither: no column sums, no fold, the workspace not touched at all
            q = _LnBwdEx(M, N, kind, mode, ws_zeroed=False)
            none = q.launch("")
            assert q.ws.untouched(), what + ": workspace touched without dw / db"
            assert C.same_bits(none["dx"].cpu(), out["dx"].cpu()), what
            _merge(worst, {"dx": q.check(none, "", what + " neither")["dx"]}, "bf16 " if mode[2] else "f32 ")


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("N", C.LN_BWD_EX_NS)
def test_layernorm_backward_narrow(N, kind):
    worst = {}
    for M in C.LN_MS:
        _ln_bwd_ex_cases(M, N, kind, C.LN_BWD_EX_MODES, worst)
    _worst("%s N=%d %s" % (C.ln_bwd_kernel(37, N, True), N, kind), worst)


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("M,N", C.LN_BWD_EX_BIG)
def test_layernorm_backward_narrow_shared_slot_rows_and_second_pass(M, N, kind):
    worst = {}
    _ln_bwd_ex_cases(M, N, kind, C.LN_BWD_EX_MODES[:2], worst)
    _worst("%s M=%d N=%d %s (%d blocks)" % (C.ln_bwd_kernel(M, N, True), M, N, kind, C.ln_bwd_grid(M, N, True)[1]),
           worst)


def test_layernorm_backward_narrow_refusals_write_nothing():
    nat = _nat()
    for name, r in C.LN_BWD_EX_REFUSED.items():
        M, N, sh = 5, r["N"], r.get("shift")
        x, w, st = In(torch.randn(M, N)), In(torch.randn(N), 1 if sh == "w" else 0), In(torch.randn(M))
        dres = In(torch.randn(M, N), 1 if sh == "dres" else 0)
        dx, dx2 = Buf(M * N, F32), Buf(M * N, BF16, shift=1 if sh == "dx2" else 0)
        dw, db, ws = Buf(N, F32), Buf(N, F32), Buf(nat.layernorm_bwd_ws_floats(N), F32)
        _refused(nat.layernorm_bwd_ex, x.ptr, 0, x.ptr, 0, w.ptr, st.ptr, st.ptr, dx.ptr, 0, dx2.ptr, dres.ptr, dw.ptr,
                 db.ptr, ws.ptr if r.get("ws", True) else 0, M, N, _st())
        assert all(b.untouched() for b in (dx, dx2, dw, db, ws)), name
        print("  refused: %s" % name)


def _ln_bwd_generic(M, N, kind, io):
    nat = _nat()
    i = C.ln_inputs(M, N, kind, io, io)
    mean, rstd = _ln_saved(M, N, kind, io)
    dy, x, w, md, rd = In(i["dy"]), In(i["x"]), In(i["w"]), In(mean), In(rstd)
    dx, dw, db = Buf(M * N, BF16 if io else F32), Buf(N, F32, init=i["dw0"]), Buf(N, F32, init=i["db0"])
    nat.layernorm_bwd(dy.ptr, x.ptr, w.ptr, md.ptr, rd.ptr, dx.ptr, dw.ptr, db.ptr, M, N, io, _st())
    torch.cuda.synchronize()
    assert dx.guard_ok() and dw.guard_ok() and db.guard_ok(), (M, N, io)
    got = {"dx": dx.cpu(M, N), "dw": dw.cpu(), "db": db.cpu()}
    return C.ln_bwd_check(got, i["dy"], i["x"], i["w"], mean, rstd, None, i["dw0"], i["db0"],
                          C.ln_bwd_adders(M, N, False), io)


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("N", C.LN_BWD_NS)
def test_layernorm_backward_generic(N, kind):
    worst = {}
    for M in C.LN_MS + tuple(m for m, n in C.LN_BWD_BIG if n == N):
        for io in (0, 1):
            _merge(worst, _ln_bwd_generic(M, N, kind, io), "bf16 " if io else "f32 ")
    _worst("layernorm_bwd_kernel N=%d %s" % (N, kind), worst)


# ---------------------------------------------------------------------------------------------- gather
def _gather_launch(c):
    src, idx = C.gather_inputs(c)
    sd, ix = In(src, c["shift"]), In(idx) if c["n_rows"] else In(torch.zeros(1, dtype=torch.int32))
    dst = Buf(max(c["n_rows"], 1) * c["row_bytes"], U8)
    return src, idx, dst, (sd.ptr, ix.ptr, dst.ptr, c["n_rows"], c["row_bytes"], _st())


@pytest.mark.parametrize("name", list(C.GATHER_CASES))
def test_gather_rows_bit_exact(name):
    c = C.GATHER_CASES[name]
    src, idx, dst, args = _gather_launch(c)
    _nat().gather_rows(*args)
    torch.cuda.synchronize()
    assert dst.guard_ok(), name
    assert torch.equal(dst.cpu(c["n_rows"], c["row_bytes"]), C.gather_ref(src, idx)), name
    print("  %s: %s, %d pass(es), equal" % (name, C.gather_kernel(c), C.gather_passes(c)))


def test_gather_rows_refusal_and_empty_write_nothing():
    for name, c in C.GATHER_REFUSED.items():
        src, idx, dst, args = _gather_launch(c)
        _refused(_nat().gather_rows, *args)
        assert dst.untouched(), name
    for name, c in C.GATHER_EMPTY.items():
        src, idx, dst, args = _gather_launch(c)
        _nat().gather_rows(*args)  # returns 0: no exception
        torch.cuda.synchronize()
        assert dst.untouched(), name
