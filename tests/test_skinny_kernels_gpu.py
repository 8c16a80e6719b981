"""dct_skinny_fwd / _dx / _dw, the fused dct_skinny_head and dct_loss_fwd_bwd[_ex], launch by launch and element by element
against the fp64 references and derived bounds of tests/skinny_cases.py.  Every comparison is kernel against reference.
Every output has guard elements after it, asserted intact; inputs carry NaN after theirs and stay unchanged; outputs
passed as null are simply absent, and the others of that launch are checked as usual.  Every test prints the worst
error / bound per tensor before it asserts <= 1; a non-finite output counts as inf.

The fused head never stores its bf16-rounded logits or dz: both roundings are charged to the bounds as errors, and that
dz is rounded is seen where one row's db IS dz (skinny_cases.head_check "dz_is_bf16").

Nothing wrong was found in these kernels: every launch of the tables below sits inside its bound.

Measured on an MI355X (2026-10-21), worst error / bound over every case (test_zz_report_worst_ratios prints them):

    dct_skinny_fwd        Y 0.990
    dct_skinny_dx         dX 0.996
    dct_skinny_dw         dW 0.178, db 0.104
    dct_skinny_head       dH 0.881, dW 0.731, db 0.543, loss 0.469, dz_is_bf16 0 (every one-row db a bf16 value)
    dct_loss_fwd_bwd      dlogits bf16 0.995, dlogits fp32 0.725, loss 0.085, correct 0
    dct_loss_fwd_bwd_ex   dlogits bf16 0.996, dlogits fp32 0.654, loss 0.052, correct 0 (exact counts, ties included)

The ratios above 0.9 are bf16 outputs (Y, dX, bf16 dlogits): the bound is the rounding to bf16 itself, and a value just
above a power of two is rounded by 2^-8 / (1 + 2^-8) of itself, 0.996 of 2^-8.  The fused head's ratios are the two
hidden bf16 roundings (z, then dz) charged as errors and pushed through the softmax and the sums: dH 0.88 is where
both land on the same side.
"""
import pytest
import torch

import skinny_cases as S

pytestmark = pytest.mark.gpu

TAIL = 16
WORST = {}
KINDS = (0, 1)


def _nat():
    from dct_amd.ops._native import native

    return native()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev():
    return torch.device("cuda", 0)


class Vec:
    """A contiguous tensor on the device with TAIL guard elements after it (fill: NaN for inputs, a value for outputs)."""

    def __init__(self, t, fill, shift=0):
        self.n, self.shape, self.fill = t.numel(), t.shape, fill
        flat = torch.full((shift + self.n + TAIL,), fill, dtype=t.dtype)
        flat[shift:shift + self.n] = t.reshape(-1)
        self.flat = flat.to(_dev())
        self.shift = shift
        self.ptr = self.flat.data_ptr() + shift * self.flat.element_size()
        self.initial = self.flat.clone()

    def data(self):
        return self.flat[self.shift:self.shift + self.n].view(self.shape)

    def tail_intact(self):
        g = self.flat[self.shift + self.n:].float()
        return bool(torch.isnan(g).all()) if self.fill != self.fill else bool((g == self.fill).all())

    def untouched(self):
        a, b = self.flat.float(), self.initial.float()
        return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _in(t):
    return Vec(t, float("nan")) if t.is_floating_point() else Vec(t, -1)


def _ratio(launcher, what, tensor, got, want, bound):
    r = S.ratio(got.detach().cpu(), want, bound)
    print("  %s %s: worst error / bound %.4f" % (what, tensor, r))
    WORST[(launcher, tensor)] = max(WORST.get((launcher, tensor), 0.0), r)
    return r


# ------------------------------------------------------------------------------------------------ skinny fwd / dx / dw
@pytest.mark.parametrize("B,K,C", S.sk_cases() + [S.SK_DX_GRID_STRIDE])
def test_skinny_fwd_dx_dw_match_fp64(B, K, C):
    nat = _nat()
    p = S.sk_problem(B, K, C)
    x, w, bias, dz = _in(p["x"]), _in(p["w"]), _in(p["bias"]), _in(p["dz"])
    what = "B=%d K=%d C=%d [CT=%d]" % (B, K, C, S.ct_of(C))
    rs = []
    for with_bias in (True, False):
        y = Vec(torch.full((B, C), -7.0, dtype=torch.bfloat16), -7.0)
        nat.skinny_fwd(x.ptr, w.ptr, bias.ptr if with_bias else 0, y.ptr, B, K, C, _st())
        torch.cuda.synchronize()
        rs.append(_ratio("dct_skinny_fwd", what + " bias=%d" % with_bias, "Y", y.data(), *S.sk_fwd_expect(p, with_bias)))
        assert y.tail_intact(), what + ": skinny_fwd wrote past Y"
    for masked in (True, False):
        dx = Vec(torch.full((B, K), -7.0, dtype=torch.bfloat16), -7.0)
        nat.skinny_dx(dz.ptr, w.ptr, x.ptr if masked else 0, dx.ptr, B, K, C, _st())
        torch.cuda.synchronize()
        rs.append(_ratio("dct_skinny_dx", what + " aux=%d" % masked, "dX", dx.data(), *S.sk_dx_expect(p, masked)))
        assert dx.tail_intact(), what + ": skinny_dx wrote past dX"
    want = S.sk_dw_expect(p)
    kb, ny, rows_per = S.dw_geometry(B, K)
    for with_db in (True, False):
        dw, db = Vec(p["dw0"], 12345.0), Vec(p["db0"], 12345.0)
        nat.skinny_dw(dz.ptr, x.ptr, dw.ptr, db.ptr if with_db else 0, B, K, C, _st())
        torch.cuda.synchronize()
        tag = what + " db=%d [%d column blocks x %d row splits of %d]" % (with_db, kb, ny, rows_per)
        rs.append(_ratio("dct_skinny_dw", tag, "dW", dw.data(), *want["dW"]))
        if with_db:
            rs.append(_ratio("dct_skinny_dw", tag, "db", db.data(), *want["db"]))
        else:
            assert db.untouched(), what + ": db written though null was passed"
        assert dw.tail_intact() and db.tail_intact(), what + ": skinny_dw wrote past dW / db"
    assert all(v.untouched() for v in (x, w, bias, dz)), what + ": an input changed"
    assert max(rs) <= 1.0, (what, rs)


def test_skinny_rejections():
    nat = _nat()
    p = S.sk_problem(3, 264, 2)
    x, w, bias, dz = _in(p["x"]), _in(p["w"]), _in(p["bias"]), _in(p["dz"])
    y = Vec(torch.full((3, 2), -7.0, dtype=torch.bfloat16), -7.0)
    dx = Vec(torch.full((3, 264), -7.0, dtype=torch.bfloat16), -7.0)
    dw, db = Vec(p["dw0"], 12345.0), Vec(p["db0"], 12345.0)
    for K, C in ((260, 2), (264, 9), (264, 0)):
        with pytest.raises(RuntimeError):
            nat.skinny_fwd(x.ptr, w.ptr, bias.ptr, y.ptr, 3, K, C, _st())
        with pytest.raises(RuntimeError):
            nat.skinny_dx(dz.ptr, w.ptr, x.ptr, dx.ptr, 3, K, C, _st())
        with pytest.raises(RuntimeError):
            nat.skinny_dw(dz.ptr, x.ptr, dw.ptr, db.ptr, 3, K, C, _st())
    with pytest.raises(RuntimeError):
        nat.skinny_fwd(x.ptr + 2, w.ptr, bias.ptr, y.ptr, 3, 264, 2, _st())
    with pytest.raises(RuntimeError):
        nat.skinny_dx(dz.ptr, w.ptr, x.ptr, dx.ptr + 2, 3, 264, 2, _st())
    with pytest.raises(RuntimeError):
        nat.skinny_dw(dz.ptr, x.ptr + 2, dw.ptr, db.ptr, 3, 264, 2, _st())
    torch.cuda.synchronize()
    assert all(v.untouched() for v in (y, dx, dw, db))


# ------------------------------------------------------------------------------------------------ fused head
@pytest.mark.parametrize("case", S.head_cases(), ids=lambda c: "B%d_K%d_C%d_%s" % (c[0], c[1], c[2], "-".join(c[4]) or "all"))
def test_skinny_head_matches_fp64(case):
    nat = _nat()
    B, K, C, mask, nulls, gs, ls = case
    p = S.head_problem(B, K, C)
    h, w, bias, y = _in(p["h"]), _in(p["w"]), _in(p["bias"]), _in(p["y"])
    what = "B=%d K=%d C=%d mask=%d null=%s [CT, NJ, NWV = %s]" % (B, K, C, mask, ",".join(nulls) or "-",
                                                                 S.head_kernel(B, K, C))
    for kind in KINDS:
        dh = Vec(torch.full((B, K), -7.0, dtype=torch.bfloat16), -7.0)
        dw, db, loss = Vec(p["dw0"], 12345.0), Vec(p["db0"], 12345.0), Vec(p["loss0"], 12345.0)
        nat.skinny_head(h.ptr, w.ptr, 0 if "bias" in nulls else bias.ptr, y.ptr, 0 if "dH" in nulls else dh.ptr, dw.ptr,
                        0 if "db" in nulls else db.ptr, 0 if "loss_sum" in nulls else loss.ptr, B, K, C, gs, kind, ls,
                        mask, _st())
        torch.cuda.synchronize()
        got = dict(dW=dw.data().cpu())
        for name, v, key in (("dH", dh, "dH"), ("db", db, "db"), ("loss_sum", loss, "loss")):
            if name in nulls:
                assert v.untouched(), what + ": %s written though null was passed" % name
            else:
                got[key] = v.data().cpu()
        r = S.head_check(got, p, kind, mask, gs, ls, "bias" not in nulls)
        for k, x in r.items():
            print("  %s kind=%d %s: worst error / bound %.4f" % (what, kind, k, x))
            WORST[("dct_skinny_head", k)] = max(WORST.get(("dct_skinny_head", k), 0.0), x)
        assert all(v.tail_intact() for v in (dh, dw, db, loss)), what + ": wrote past an output"
        assert all(v.untouched() for v in (h, w, bias, y)), what + ": an input changed"
        assert all(x <= 1.0 for x in r.values()), (what, kind, r)


def test_skinny_head_supported_and_rejections():
    nat = _nat()
    for K, C in S.HEAD_SUPPORT:
        assert bool(nat.skinny_head_supported(K, C)) == S.head_supported(K, C), (K, C)
    p = S.head_problem(5, 512, 2)
    h, w, bias, y = _in(p["h"]), _in(p["w"]), _in(p["bias"]), _in(p["y"])
    dh = Vec(torch.full((5, 512), -7.0, dtype=torch.bfloat16), -7.0)
    dw, db, loss = Vec(p["dw0"], 12345.0), Vec(p["db0"], 12345.0), Vec(p["loss0"], 12345.0)
    for what, o in S.HEAD_REJECTED:
        ptr = dict(H=h.ptr, labels=y.ptr, dW=dw.ptr, dH=dh.ptr)
        if "null" in o:
            ptr[o["null"]] = 0
        if "shift" in o:
            ptr[o["shift"]] += 2
        with pytest.raises(RuntimeError):
            nat.skinny_head(ptr["H"], w.ptr, bias.ptr, ptr["labels"], ptr["dH"], ptr["dW"], db.ptr, loss.ptr, 5,
                            o.get("K", 512), o.get("C", 2), 0.2, 0, 0.2, 1, _st())
        print("  refused: " + what)
    torch.cuda.synchronize()
    assert all(v.untouched() for v in (dh, dw, db, loss))


# ------------------------------------------------------------------------------------------------ loss kernel
def _loss_launch(nat, p, lbf16, kind, gs, ls, nulls, ex):
    M, C = p["z"].shape
    z, y = _in(p["z"]), _in(p["y"])
    dl = Vec(torch.full((M, C), -7.0, dtype=p["z"].dtype), -7.0)
    loss, correct = Vec(p["loss0"], 12345.0), Vec(p["correct0"], 12345.0)
    args = (z.ptr, lbf16, y.ptr, 0 if "dlogits" in nulls else dl.ptr, 0 if "loss_sum" in nulls else loss.ptr,
            0 if "correct_sum" in nulls else correct.ptr, M, C, gs, kind)
    if ex:
        nat.loss_fwd_bwd_ex(*args, ls, _st())
    else:
        nat.cross_entropy_fwd_bwd(*args, _st())
    torch.cuda.synchronize()
    launcher = "dct_loss_fwd_bwd_ex" if ex else "dct_loss_fwd_bwd"
    what = "M=%d C=%d bf16=%d kind=%d null=%s [%s, %d blocks x %d rows per thread]" % (
        (M, C, lbf16, kind, ",".join(nulls) or "-", S.loss_path(C)) + S.loss_geometry(M))
    want = S.loss_expect(p, kind, gs, ls if ex else 1.0, lbf16)
    rs = []
    for name, v, key in (("dlogits", dl, "dlogits"), ("loss_sum", loss, "loss"), ("correct_sum", correct, "correct")):
        if name in nulls:
            assert v.untouched(), what + ": %s written though null was passed" % name
        else:
            label = key if key != "dlogits" else "dlogits " + ("bf16" if lbf16 else "fp32")
            rs.append(_ratio(launcher, what, label, v.data(), *want[key]))
        assert v.tail_intact(), what + ": wrote past " + name
    assert z.untouched() and y.untouched(), what + ": an input changed"
    assert max(rs) <= 1.0, (what, rs)


@pytest.mark.parametrize("lbf16", [0, 1])
@pytest.mark.parametrize("C", S.LOSS_CS)
def test_loss_matches_fp64(C, lbf16):
    """Both loss kinds, both entry points (loss_scale 1 and 1/3), every null argument, M = 1 and 1000; ties for the
    maximum and logits out to +-30 are in the inputs."""
    nat = _nat()
    for M in S.LOSS_MS:
        p = S.loss_problem(M, C, lbf16)
        for kind in KINDS:
            for nulls in S.LOSS_NULLS:  # every null argument with both loss kinds, through both entry points
                for ex in (False, True):
                    _loss_launch(nat, p, lbf16, kind, 1.0 / 3.0 if ex else 1.0 / M, 1.0 / 3.0, nulls, ex)


@pytest.mark.parametrize("C,lbf16,kind", S.LOSS_BIG)
def test_loss_grid_stride_pass(C, lbf16, kind):
    """M = 262144 + 5: five rows run in a second pass of the 1024-workgroup grid."""
    p = S.loss_problem(S.LOSS_BIG_M, C, lbf16)
    _loss_launch(_nat(), p, lbf16, kind, 1.0 / S.LOSS_BIG_M, 1.0 / 3.0, (), True)


def test_zz_report_worst_ratios():
    """The worst error / bound per launcher and tensor over this module's run (the figures of the docstring)."""
    for (launcher, tensor), r in sorted(WORST.items()):
        print("WORST %-24s %-10s %.4f" % (launcher, tensor, r))
    assert all(r <= 1.0 for r in WORST.values())
