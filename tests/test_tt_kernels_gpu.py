"""The TabTransformer step's kernels, each launcher on its own, stage by stage and element by element against the fp64
references and derived bounds of tests/tt_cases.py: the block forward in every mode (all stored; qkv / f / pre not
stored; inference; pooled; embedded; gathered), the block backward in every mode (stored and recomputed pre and qkv,
direct atomics and LayerNorm replicas, dout rows and dpool, embedded; the three combinations models/tabtransformer.py
runs and four no caller uses), the launchers' rejections, the embedding and its gradients (on their own and riding in
the grouped dW launch) and the classifier head (forward, backward, fused; 4 and 16 samples per workgroup).  Every
comparison is kernel against reference on the CPU; where the source states two modes bit-identical that is asserted as
well.  Every test prints its worst error / bound ratio per tensor before it asserts <= 1; every output buffer has a
guard region after it.

Measured on an MI355X (2026-10-20): worst error / bound per tensor over B = 1, 3, 17, 37; "unit / edge" input sets.

  forward, all stored (as launched by ops/nn.py, pooled, embedded and gathered launches within 0.02 of these; what they
  share with the all-stored launch is bit-identical to it):
    mean1 0.015 / 0.015   rstd1 0.029 / 0.253   a1 0.993 / 0.993   qkv 0.993 / 0.993   o 0.757 / 0.830
    lse 0.087 / 0.049     h1 0.056 / 0.036 (embedded 0.107, gathered 0.146: the fmaf's u |h| is most of that bound)
    mean2 0.018 / 0.016   rstd2 0.027 / 0.032   a2 0.993 / 0.994   pre 0.994 / 0.993   f 0.992 / 0.993
    out 0.011 / 0.009     pool 0.001 / 0.001    wT bit-equal
  backward, stored (recomputed pre / qkv, replicas and the three model combinations give the same figures: every
  launch's dout16, dpre, dh1_16, dqkv, dh and dh16 are asserted bit-identical to the launch on the same inputs that
  stores everything; dpool and embedded launches: dqkv 0.54 - 0.89, the rest within 0.02):
    dpre 0.993 / 0.993    dh1_16 0.976 / 0.980  dqkv 0.625 / 0.857 (dpool: 0.885)   dh 0.003 / 0.009
    dln1_w, dln1_b, dln2_w, dln2_b <= 0.003     dout16, dh16 bit-equal
  embedding: h 0.996, dE 0.795, dc 0.505 (B = 1: one product, one add); riding in the grouped dW launch dE 0.146,
  dc 0.111, the four dW 0.021, their column sums 0.005
  head (T = 64 and 3 | T = 1): loss 0.002 | 0.002, dh 0.003 | 0.002, dln_w 0.152 | 0.115, dln_b 0.029 | 0.039,
  dW 0.124 | 0.078, dbias 0.008 | 0.007; dh16 bit-equal; tt_head_fused the same figures, its loss bit-equal

Above 0.9, each by its own final rounding and nothing to watch: a1, qkv, a2, pre, f, dpre, dh1_16 (bf16 outputs whose
bound is 2^-8 |value| plus an fp32 accumulation term hundreds of times smaller: the worst element sits next to a
rounding tie, 2^-8 / (1 + 2^-8) of |value| at worst; the torch emulation of tests/test_tt_cases_cpu.py gives the same
figures) and the embedding's h (one fmaf: u |h|).  o and dqkv carry the hidden bf16 roundings of P, do and dS in
their bounds and stay at 0.6 - 0.9, where the emulation also is (0.60 - 0.83 and 0.42 - 0.89).  The fp32 outputs (h1,
out, pool, dh, the parameter gradients, the head) stay below 0.16: their bounds charge every accumulation step a
rounding of the whole sum of magnitudes.

One finding: the forward launcher in inference mode (a1 null) still handed layer_norm_rows the caller's mean / rstd
buffers, which the kernel then wrote; dct_tt_block_fwd* now withholds them (csrc/tt_block.hip, host side only).
"""
import functools

import pytest
import torch

import tt_cases as C

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = {torch.float32: -7.25, torch.bfloat16: -7.0, torch.int64: -77, torch.int32: -77}
F32, BF16 = torch.float32, torch.bfloat16
T, DM, NH, FF = C.T, C.DM, C.NH, C.FF


def _nat():
    from dct_amd.ops._native import native

    return native()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev():
    return torch.device("cuda", 0)


class Buf:
    """An output buffer of n elements, guard-filled, with GUARD more elements after it."""

    def __init__(self, n, dtype, init=None):
        self.n, self.fill = n, FILL[dtype]
        self.all = torch.full((n + GUARD,), self.fill, dtype=dtype, device=_dev())
        if init is not None:
            self.all[:n] = init.reshape(-1).to(_dev())
        self.t = self.all[:n]

    @property
    def ptr(self):
        return self.all.data_ptr()

    def guard_ok(self):
        return bool((self.all[self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.all == self.fill).all())

    def cpu(self, *shape):
        return self.t.cpu().reshape(*shape) if shape else self.t.cpu()


def _worst(what, ratios, keys=None):
    keys = list(ratios) if keys is None else keys
    print("  %s: %s" % (what, "  ".join("%s %.3f" % (k, ratios[k]) for k in keys)))
    bad = {k: ratios[k] for k in keys if not ratios[k] <= 1.0}
    assert not bad, (what, bad)


@functools.lru_cache(maxsize=None)
def _params(kind):
    """(CPU, device) copies of the block's parameters; nothing changes them."""
    p = C.block_params(kind)
    return p, {k: v.to(_dev()) for k, v in p.items()}


FWD_SHAPES = {"a1": (BF16, DM), "mean1": (F32, 1), "rstd1": (F32, 1), "qkv": (BF16, 3 * DM), "o": (BF16, DM),
              "lse": (F32, None), "h1": (F32, DM), "a2": (BF16, DM), "mean2": (F32, 1), "rstd2": (F32, 1),
              "f": (BF16, FF), "pre": (BF16, FF), "out": (F32, DM), "wT": (BF16, None)}


def _fwd_bufs(B):
    M = B * T
    n = {"lse": B * NH * T, "wT": C.WT_TOTAL}
    bufs = {k: Buf(n.get(k, M * (w or 1)), dt) for k, (dt, w) in FWD_SHAPES.items()}
    bufs["pool"] = Buf(B * DM, F32)
    return bufs


def _fwd_host(bufs, B):
    out = {}
    for k, b in bufs.items():
        w = FWD_SHAPES[k][1] if k in FWD_SHAPES else DM
        out[k] = b.cpu(-1, w) if w and w > 1 else b.cpu()
    return out


def _fwd_launch(kind, B, spec, h=None, emb=None, gx=None, bufs=None):
    """One forward launch as ``spec`` (a tt_cases.FWD_MODES / FWD_REJECTED description) says; returns the buffers.
    ``h`` / ``emb``: device tensors; ``gx``: the 11 gather values (gx[5] is the embedding's x)."""
    nat, (_, pd) = _nat(), _params(kind)
    bufs = bufs or _fwd_bufs(B)
    null, mis = set(spec.get("null", ())), set(spec.get("misaligned", ()))
    addr = {k: pd[k].data_ptr() for k in C.FWD_PTRS[1:13]}
    addr["h"] = h.data_ptr() if h is not None else 0
    addr.update({k: bufs[k].ptr for k in C.FWD_OUTPUTS})
    ptrs = [0 if k in null else addr[k] + (4 if k in mis else 0) for k in C.FWD_PTRS]
    dims = spec.get("dims", (T, DM, NH, FF))
    pool = (bufs["pool"].ptr + (4 if "pool" in mis else 0)) if spec.get("pool") else 0
    args = (ptrs, B, dims[0], dims[1], dims[2], dims[3], C.EPS, C.SCALE)
    if spec.get("embed"):
        en = spec.get("embed_null", ())
        em = [0 if n in en else t.data_ptr() for n, t in zip(("ex", "eE", "ec"), emb)]
        if spec.get("gather"):
            nat.tt_block_fwd_gx(*args, pool, *em, gx, _st())
        else:
            nat.tt_block_fwd_ex(*args, pool, *em, _st())
    elif spec.get("pool"):
        nat.tt_block_fwd_ex(*args, pool, 0, 0, 0, _st())
    else:
        nat.tt_block_fwd(*args, _st())
    torch.cuda.synchronize()
    return bufs


def _guards(what, bufs, written):
    """Guards intact after every buffer; buffers outside ``written`` untouched."""
    for k, b in bufs.items():
        assert b.guard_ok(), "%s: wrote past the end of %s" % (what, k)
        if k not in written:
            assert b.untouched(), "%s: %s written" % (what, k)


def _written(spec):
    null = set(spec["null"])
    if "a1" in null:
        return {"out"} | ({"pool"} if spec["pool"] else set())
    return (set(C.FWD_OUTPUTS) - null) | ({"pool"} if spec["pool"] else set())


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("B", list(C.BLOCK_BS))
def test_block_forward_stages_in_every_plain_mode(B, kind):
    """All stored; qkv / f / pre not stored (as ops/nn.py launches it); inference; pool with and without out."""
    p, _ = _params(kind)
    h = C.block_input(B, kind)
    hd = h.to(_dev())
    stored = None
    for mode in ("stored", "as_launched", "inference", "pool_only", "pool_and_out"):
        spec = C.FWD_MODES[mode]
        bufs = _fwd_launch(kind, B, spec, h=hd)
        wr = _written(spec)
        _guards(mode, bufs, wr)
        got = {k: v for k, v in _fwd_host(bufs, B).items() if k in wr}
        if stored is None:
            stored = got
        else:  # what this mode does not store, for the stage references: the all-stored launch's
            for k in wr & set(stored):
                assert C.same_bits(got[k], stored[k]), "%s: %s differs from the all-stored launch" % (mode, k)
        r = C.fwd_check({**stored, **got, "out": got.get("out"), "pool": got.get("pool")}, p, h=h)
        _worst("fwd %s B=%d %s" % (mode, B, kind), r, [k for k in r if k in wr])


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("B", list(C.BLOCK_BS))
def test_block_forward_embedded(B, kind):
    """The first block's input computed from the features: x E + c in fp64 as the input reference, and h1
    bit-identical to the plain launch on tt_embed_fwd's output (the same fmaf)."""
    nat, (p, _) = _nat(), _params(kind)
    emb = C.embed_input(B, kind)
    embd = [t.to(_dev()) for t in emb]
    hk = Buf(B * T * DM, F32)
    nat.tt_embed_fwd(embd[0].data_ptr(), embd[1].data_ptr(), embd[2].data_ptr(), hk.ptr, B, T, DM, _st())
    plain = _fwd_launch(kind, B, C.FWD_MODES["stored"], h=hk.t)
    assert hk.guard_ok()
    spec = C.FWD_MODES["embedded"]
    bufs = _fwd_launch(kind, B, spec, emb=embd)
    _guards("embedded", bufs, _written(spec))
    got = _fwd_host(bufs, B)
    got["pool"] = None
    _worst("fwd embedded B=%d %s" % (B, kind), C.fwd_check(got, p, emb=emb))
    for k in C.FWD_OUTPUTS:
        assert C.same_bits(bufs[k].t, plain[k].t), "embedded: %s differs from the plain launch on tt_embed_fwd's h" % k


@pytest.mark.parametrize("B", list(C.BLOCK_BS))
def test_block_forward_gathered(B):
    """dct_tt_block_fwd_gx: the batch gathered from the dataset (cursor 0 inside the list, cursor 2 wrapping mid-batch;
    a permutation and a list with repeats), labels, step counter, the zero range - and the block itself."""
    kind = "unit"
    p, _ = _params(kind)
    stride, n_items, _, cursors = C.batch_geometry(B)
    X, Y, lists = C.gather_inputs(B)
    _, E, c = C.embed_input(B, kind)
    Xd, Yd, Ed, cd = (t.to(_dev()) for t in (X, Y, E, c))
    zn = C.gx_zero_ns(B)
    assert cursors == (0, 2)
    # (index list, cursor, zero_n, with a step counter, with a zero range): null ones are accepted
    cases = [("permutation", 0, zn[0], True, True), ("permutation", 2, zn[1], False, True),
             ("repeated", 0, zn[2], True, False), ("repeated", 2, zn[3], True, True),
             ("permutation", 2, zn[4], True, True), ("repeated", 0, zn[2], True, True)]
    for name, cursor, zero_n, with_counter, with_zero in cases:
        idx = lists[name]
        idxd = idx.to(_dev())
        rows = C.gather_rows_ref(idx, cursor, stride, n_items, B)
        xdst, ydst = Buf(B * T, F32), Buf(B, torch.int64)
        step, zero = Buf(1, torch.int32, torch.tensor([41])), Buf(zero_n, F32)
        cur = torch.tensor([cursor], dtype=torch.int32, device=_dev())
        gx = [Xd.data_ptr(), idxd.data_ptr(), cur.data_ptr(), stride, n_items, xdst.ptr, Yd.data_ptr(), ydst.ptr,
              step.ptr if with_counter else 0, zero.ptr if with_zero else 0, zero_n]
        spec = C.FWD_MODES["gathered"]
        what = "gathered %s cursor %d zero_n %d" % (name, cursor, zero_n)
        bufs = _fwd_launch(kind, B, spec, emb=(xdst.t, Ed, cd), gx=gx)
        _guards(what, bufs, _written(spec))
        assert xdst.guard_ok() and ydst.guard_ok() and step.guard_ok() and zero.guard_ok(), what
        assert C.same_bits(xdst.cpu(B, T), X[rows]), what + ": gathered rows"
        assert torch.equal(ydst.cpu(), Y[rows]), what + ": labels"
        assert int(step.t[0]) == (42 if with_counter else 41), what + ": step counter"
        assert zero.untouched() if not with_zero else bool((zero.t == 0).all()), what + ": zero range"
        emb = (X[rows], E, c)
        got = _fwd_host(bufs, B)
        got["pool"] = None
        _worst("fwd %s B=%d" % (what, B), C.fwd_check(got, p, emb=emb))
        ref = _fwd_launch(kind, B, C.FWD_MODES["embedded"], emb=[t.to(_dev()) for t in emb])
        for k in C.FWD_OUTPUTS:
            assert C.same_bits(bufs[k].t, ref[k].t), what + ": %s differs from the embedded launch" % k


def test_block_forward_rejections():
    kind, B = "unit", 3
    hd = C.block_input(B, kind).to(_dev())
    x, E, c = (t.to(_dev()) for t in C.embed_input(B, kind))
    X, Y, lists = C.gather_inputs(B)
    stride, n_items, _, _ = C.batch_geometry(B)
    keep = [t.to(_dev()) for t in (X, lists["permutation"], torch.zeros(1, dtype=torch.int32), Y)]
    for name, rej in C.FWD_REJECTED.items():
        spec = dict(C.FWD_MODES[rej["base"]], **{k: v for k, v in rej.items() if k != "base"})
        bufs, ydst, other = _fwd_bufs(B), Buf(B, torch.int64), Buf(B * T, F32)
        gx = None
        if spec["gather"]:
            xd = Buf(B * T, F32)
            gx = [keep[0].data_ptr(), 0 if "idx" in spec.get("gx_null", ()) else keep[1].data_ptr(), keep[2].data_ptr(),
                  stride, n_items, xd.ptr if spec.get("gx5_is_ex", True) else other.ptr, keep[3].data_ptr(), ydst.ptr,
                  0, 0, 0][:spec.get("n_gx", 11)]
            emb = (xd.t, E, c)
        else:
            emb = (x, E, c)
        with pytest.raises(RuntimeError):
            _fwd_launch(kind, B, spec, h=hd, emb=emb, gx=gx, bufs=bufs)
        torch.cuda.synchronize()
        _guards("rejected: " + name, bufs, set())
        assert ydst.untouched() and other.untouched(), name


# ---------------------------------------------------------------------------------------------- backward
BWD_SHAPES = {"dpre": (BF16, FF), "dh1_16": (BF16, DM), "dqkv": (BF16, 3 * DM), "dh": (F32, DM), "dh16": (BF16, DM),
              "dout16": (BF16, DM)}
LN_GRADS = ("dln1_w", "dln1_b", "dln2_w", "dln2_b")


def _bwd_bufs(B, init):
    bufs = {k: Buf(B * T * w, dt) for k, (dt, w) in BWD_SHAPES.items()}
    bufs.update({k: Buf(DM, F32, init[k]) for k in LN_GRADS})
    return bufs


def _bwd_launch(kind, B, spec, saved, bufs, dout=None, dpool=None, emb=None):
    """One backward launch as ``spec`` says on the device tensors ``saved`` of a forward launch, into ``bufs``; returns
    the replica workspace + ticket (None without them)."""
    nat, (_, pd) = _nat(), _params(kind)
    null, mis = set(spec.get("null", ())), set(spec.get("misaligned", ()))
    addr = {k: saved[k].data_ptr() for k in ("mean1", "rstd1", "qkv", "o", "lse", "h1", "mean2", "rstd2", "pre", "wT",
                                             "a2")}
    addr.update(dout=dout.data_ptr() if dout is not None else 0, h=saved["h"].data_ptr() if "h" in saved else 0,
                ln1_w=pd["ln1_w"].data_ptr(), ln2_w=pd["ln2_w"].data_ptr(), w1=pd["w1"].data_ptr(),
                b1=pd["b1"].data_ptr())
    addr.update({k: bufs[k].ptr for k in C.BWD_OUTPUTS})
    if spec["ext"] and spec["recomp"]:
        null.add("pre")
    if spec["qkv_recomp"]:
        null.add("qkv")
    if spec["pooled"]:
        null.add("dout")
    if spec["embed"]:
        null |= {"h", "dh16"}
    if spec["dpre_null"]:
        null.add("dpre")
    names = C.BWD_PTRS[:26 if spec["ext"] else 23]
    ptrs = [0 if k in null else addr[k] + (4 if k in mis else 0) for k in names]
    rep = None
    if spec["lnrep"]:
        rep = torch.zeros(C.LN_REP * 4 * DM + 4 + GUARD, dtype=F32, device=_dev())
        rep[C.LN_REP * 4 * DM + 4:] = FILL[F32]
    ticket = spec.get("ticket", spec["lnrep"])
    dims = spec.get("dims", (T, DM, NH, FF))
    em = [t.data_ptr() for t in emb] if spec["embed"] else [0, 0, 0]
    qr = [saved["a1"].data_ptr(), pd["wqkv"].data_ptr(), pd["bqkv"].data_ptr()] if spec["qkv_recomp"] else [0, 0, 0]
    nat.tt_block_bwd_ex(ptrs, B, dims[0], dims[1], dims[2], dims[3], C.SCALE,
                        dpool.data_ptr() if spec["pooled"] else 0,
                        bufs["dout16"].ptr if spec["pooled"] and spec.get("dout16", True) else 0, *em,
                        rep.data_ptr() if rep is not None else 0,
                        rep[C.LN_REP * 4 * DM:].data_ptr() if ticket else 0, *qr, _st())
    torch.cuda.synchronize()
    return rep


def _saved_dev(bufs, **more):
    s = {k: b.t for k, b in bufs.items()}
    s.update(more)
    return s


@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("B", list(C.BLOCK_BS))
def test_block_backward_stages_in_every_mode(B, kind):
    """Every tt_cases.BWD_MODES entry on the saved tensors of the kernel's own forward launch (lse belongs to qkv),
    against the stage references; and what is not an atomic sum (tt_cases.BWD_SAME_BITS) bit-identical to the launch
    on the same inputs that stores everything: recomputed pre and q / k / v and the replicas change no bit."""
    p, _ = _params(kind)
    h, emb = C.block_input(B, kind), C.embed_input(B, kind)
    hd, embd = h.to(_dev()), [t.to(_dev()) for t in emb]
    fwd = {False: _fwd_launch(kind, B, C.FWD_MODES["stored"], h=hd),
           True: _fwd_launch(kind, B, C.FWD_MODES["embedded"], emb=embd)}
    host = {e: _fwd_host(b, B) for e, b in fwd.items()}
    host[False]["h"] = h
    dout, dpool, init = C.dout_input(B, kind), C.dout_input(B, kind, pooled=True), C.ln_grad_init()
    doutd, dpoold = dout.to(_dev()), dpool.to(_dev())
    base = {}  # mode -> its non-atomic outputs, for the launches on the same inputs to be bit-compared with
    for mode, spec in C.BWD_MODES.items():
        e, pooled = spec["embed"], spec["pooled"]
        saved = _saved_dev(fwd[e], **({} if e else {"h": hd}))
        bufs = _bwd_bufs(B, init)
        rep = _bwd_launch(kind, B, spec, saved, bufs, dout=doutd, dpool=dpoold, emb=embd)
        written = set(C.BWD_OUTPUTS) - ({"dh16"} if e else set()) - ({"dpre"} if spec["dpre_null"] else set()) \
            | ({"dout16"} if pooled else set())
        for k in BWD_SHAPES:
            assert bufs[k].guard_ok(), "%s: wrote past the end of %s" % (mode, k)
            assert k in written or bufs[k].untouched(), "%s: %s written" % (mode, k)
        for k in LN_GRADS:
            assert bufs[k].guard_ok(), "%s: wrote past the end of %s" % (mode, k)
        if spec["lnrep"]:
            assert bool((rep[:C.LN_REP * 4 * DM + 4] == 0).all()), mode + ": replicas / ticket not zero afterwards"
            assert bool((rep[C.LN_REP * 4 * DM + 4:] == FILL[F32]).all()), mode + ": wrote past the ticket"
        got = {k: bufs[k].cpu(-1, BWD_SHAPES[k][1]) for k in BWD_SHAPES if k in written}
        got.update({k: bufs[k].cpu() for k in LN_GRADS})
        sv = dict(host[e])
        first = C.bwd_base_mode(mode)
        if first == mode:
            assert not (spec["recomp"] or spec["qkv_recomp"] or spec["lnrep"] or spec["dpre_null"]), mode
            base[mode] = {k: got[k] for k in C.BWD_SAME_BITS if k in written}
        else:  # stored or recomputed, direct or through the replicas: the same bits (the source says so)
            same = [k for k in C.BWD_SAME_BITS if k in written]
            assert same and set(same) == set(base[first]) - ({"dpre"} if spec["dpre_null"] else set()), (mode, same)
            for k in same:
                assert C.same_bits(got[k], base[first][k]), "%s: %s differs from the %s launch" % (mode, k, first)
            print("  bwd %s B=%d %s: %s bit-equal to %s" % (mode, B, kind, " ".join(same), first))
        if spec["dpre_null"]:  # what this launch does not store: the launch's that does
            sv["dpre"] = base[first]["dpre"]
        r = C.bwd_check(got, sv, p, init=init, **({"dpool": dpool} if pooled else {"dout": dout}),
                        **({"emb": emb} if e else {}))
        assert set(r) == written | set(LN_GRADS), (mode, sorted(r))
        _worst("bwd %s B=%d %s" % (mode, B, kind), r)


def test_block_backward_rejections():
    kind, B = "unit", 3
    hd = C.block_input(B, kind).to(_dev())
    fwd = _fwd_launch(kind, B, C.FWD_MODES["stored"], h=hd)
    saved = _saved_dev(fwd, h=hd)
    doutd, dpoold = C.dout_input(B, kind).to(_dev()), C.dout_input(B, kind, pooled=True).to(_dev())
    init = C.ln_grad_init()
    for name, rej in C.BWD_REJECTED.items():
        spec = dict(C.BWD_MODES[rej["base"]], **{k: v for k, v in rej.items() if k != "base"})
        bufs = _bwd_bufs(B, init)
        with pytest.raises(RuntimeError):
            _bwd_launch(kind, B, spec, saved, bufs, dout=doutd, dpool=dpoold)
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert b.guard_ok(), (name, k)
            assert C.same_bits(b.cpu(), init[k]) if k in LN_GRADS else b.untouched(), (name, k)


# ---------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("kind", C.INPUT_SETS)
@pytest.mark.parametrize("F", C.EMBED_FS)
@pytest.mark.parametrize("B", C.EMBED_BS)
def test_embedding_forward_and_backward(B, F, kind):
    nat = _nat()
    x, E, c = C.embed_input(B, kind, F=F)
    xd, Ed, cd = (t.to(_dev()) for t in (x, E, c))
    h = Buf(B * F * DM, F32)
    nat.tt_embed_fwd(xd.data_ptr(), Ed.data_ptr(), cd.data_ptr(), h.ptr, B, F, DM, _st())
    torch.cuda.synchronize()
    assert h.guard_ok()
    g = torch.Generator().manual_seed(B + F)
    dh, dE0, dc0 = (torch.randn(*s, generator=g) for s in ((B * F, DM), (F, DM), (F, DM)))
    if kind == "edge":
        dh = dh * 10.0 ** (-4.0 * torch.rand(B * F, DM, generator=g))
    dE, dc, dhd = Buf(F * DM, F32, dE0), Buf(F * DM, F32, dc0), dh.to(_dev())
    nat.tt_embed_bwd(xd.data_ptr(), dhd.data_ptr(), dE.ptr, dc.ptr, B, F, DM, _st())
    torch.cuda.synchronize()
    assert dE.guard_ok() and dc.guard_ok()
    rE, eE, rc, ec = C.embed_bwd_ref(x, dh, dE0, dc0)
    _worst("embed B=%d F=%d %s" % (B, F, kind),
           {"h": C.ratio(h.cpu(-1, DM), *C.embed_ref(x, E, c)), "dE": C.ratio(dE.cpu(F, DM), rE, eE),
            "dc": C.ratio(dc.cpu(F, DM), rc, ec)})


@pytest.mark.parametrize("F", C.EMBED_FS)
@pytest.mark.parametrize("B", C.EMBED_BS + (17,))
def test_grouped_dw_with_the_embedding_gradients_riding(B, F):
    """dct_gemm_bf16_dw_grouped_embed on a block's four dW problems over B * 64 rows: the four products and column
    sums against gemm_ref and, from 8 k-tiles on, dE / dc riding in the same launch; below that the launcher says the
    ride did not run and leaves dE / dc alone."""
    nat, K = _nat(), B * T
    g = torch.Generator().manual_seed(100 + B + F)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    shapes = [(DM, FF), (FF, DM), (DM, DM), (3 * DM, DM)]  # (columns of dZ, columns of X): W2, W1, Wo, Wqkv
    dz = [C.bf(r(K, m)) for m, _ in shapes]
    xs = [C.bf(r(K, n)) for _, n in shapes]
    c0, s0 = [r(m, n) for m, n in shapes], [r(m) for m, _ in shapes]
    cb = [Buf(m * n, F32, c0[i]) for i, (m, n) in enumerate(shapes)]
    sb = [Buf(m, F32, s0[i]) for i, (m, _) in enumerate(shapes)]
    x, _, _ = C.embed_input(B, "unit", F=F)
    dh, dE0, dc0 = r(B * F, DM), r(F, DM), r(F, DM)
    dE, dc = Buf(F * DM, F32, dE0), Buf(F * DM, F32, dc0)
    dev = [t.to(_dev()) for t in dz + xs + [x, dh]]
    rode = nat.gemm_bf16_dw_grouped_embed([t.data_ptr() for t in dev[:4]], [t.data_ptr() for t in dev[4:8]],
                                          [b.ptr for b in cb], [m for m, _ in shapes], [n for _, n in shapes], K,
                                          [b.ptr for b in sb], 1, dev[8].data_ptr(), dev[9].data_ptr(), dE.ptr, dc.ptr,
                                          B, F, _st())
    torch.cuda.synchronize()
    assert rode == C.grouped_ride_runs(B)
    ratios = {}
    for i, (m, n) in enumerate(shapes):
        assert cb[i].guard_ok() and sb[i].guard_ok()
        ref, ab = C.gemm_ref(dz[i].t(), xs[i])
        ratios["dW%d" % i] = C.ratio(cb[i].cpu(m, n), c0[i].double() + ref, C.dw_bound(ref, ab, K, c0[i].double()))
        cs, cabs = dz[i].double().sum(0), dz[i].double().abs().sum(0)
        ratios["colsum%d" % i] = C.ratio(sb[i].cpu(), s0[i].double() + cs, C.dw_bound(cs, cabs, K, s0[i].double()))
    assert dE.guard_ok() and dc.guard_ok()
    if rode:
        rE, eE, rc, ec = C.embed_bwd_ref(x, dh, dE0, dc0)
        ratios["dE"], ratios["dc"] = C.ratio(dE.cpu(F, DM), rE, eE), C.ratio(dc.cpu(F, DM), rc, ec)
    else:
        assert C.same_bits(dE.cpu(F, DM), dE0) and C.same_bits(dc.cpu(F, DM), dc0)
    _worst("grouped dW B=%d F=%d" % (B, F), ratios)


# ---------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("Tn", C.HEAD_TS)
@pytest.mark.parametrize("B", C.HEAD_BS)
def test_head_forward_backward_and_fused(B, Tn):
    """tt_head_fwd, tt_head_bwd (dloss != 1 on the edge set) and tt_head_fused for every C and both input sets:
    T = 64 and 3 take 4 samples per workgroup, T = 1 sixteen."""
    nat = _nat()
    for kind in C.INPUT_SETS:
        for Cn in C.HEAD_CS:
            i = C.head_inputs(B, Tn, Cn, kind)
            d = {k: i[k].to(_dev()) for k in ("h", "y", "ln_w", "ln_b", "W", "bias", "dloss")}
            base = [d[k].data_ptr() for k in ("h", "y", "ln_w", "ln_b", "W", "bias")]
            nparts = -(-B // (C.HEAD_SPB_POOLED if Tn == 1 else C.HEAD_SPB))
            partial, ticket = Buf(-(-B // C.HEAD_SPB), F32), Buf(1, torch.int32, torch.tensor([0]))
            what = "head B=%d T=%d C=%d %s" % (B, Tn, Cn, kind)
            losses = []
            for _ in range(3):  # one scratch, three launches: the ticket returns to zero, the loss is bit-identical
                loss = Buf(1, F32)
                nat.tt_head_fwd(base + [loss.ptr, partial.ptr, ticket.ptr], B, Tn, DM, Cn, C.EPS, _st())
                torch.cuda.synchronize()
                assert int(ticket.t[0]) == 0 and ticket.guard_ok() and loss.guard_ok() and partial.guard_ok(), what
                assert bool((partial.t[nparts:] == FILL[F32]).all()), what + ": partials past the grid"
                losses.append(loss.cpu())
            assert C.same_bits(losses[0], losses[1]) and C.same_bits(losses[0], losses[2]), what

            def grads():
                init = i["init"]
                return dict(dh=Buf(B * Tn * DM, F32), dh16=Buf(B * Tn * DM, BF16), dln_w=Buf(DM, F32, init["dln_w"]),
                            dln_b=Buf(DM, F32, init["dln_b"]), dW=Buf(Cn * DM, F32, init["dW"]),
                            dbias=Buf(Cn, F32, init["dbias"]))

            def host(g, **more):
                assert all(b.guard_ok() for b in g.values()), what
                out = {k: g[k].cpu(-1, DM) for k in ("dh", "dh16", "dW")}
                out.update({k: g[k].cpu() for k in ("dln_w", "dln_b", "dbias")}, **more)
                return out

            order = ("dh", "dh16", "dln_w", "dln_b", "dW", "dbias")
            g = grads()
            nat.tt_head_bwd(base + [d["dloss"].data_ptr()] + [g[k].ptr for k in order], B, Tn, DM, Cn, C.EPS, _st())
            torch.cuda.synchronize()
            dl = float(i["dloss"])
            _worst(what + " fwd + bwd", C.head_check(host(g, loss=losses[0]), i, B, Tn, Cn, dl))
            fused = []
            for _ in range(3):
                g, loss = grads(), Buf(1, F32)
                nat.tt_head_fused(base + [loss.ptr, partial.ptr, ticket.ptr] + [g[k].ptr for k in order], B, Tn, DM,
                                  Cn, C.EPS, _st())
                torch.cuda.synchronize()
                assert int(ticket.t[0]) == 0 and loss.guard_ok() and partial.guard_ok(), what
                fused.append(host(g, loss=loss.cpu()))
            _worst(what + " fused", C.head_check(fused[0], i, B, Tn, Cn, 1.0))
            assert C.same_bits(fused[0]["loss"], losses[0]), what + ": the fused loss differs from tt_head_fwd's"
            for k in ("loss", "dh", "dh16"):  # (the parameter gradients are atomics: order may differ)
                assert C.same_bits(fused[0][k], fused[1][k]) and C.same_bits(fused[0][k], fused[2][k]), (what, k)
