"""Two parts of mlp_block5's step schedule (csrc/mlp_block5_impl.h), emulated on the host in float32.

The logit-share reduce-scatter: the two logit shares of a lane were all-reduced over lane bits 2..5 (bku::sum_bits2to5) and only
the one of class cb = lane bit 2 was stored; now the lane keeps its class, sends the other through row_ror:4
and runs the same three further levels.  The emulation follows the cross-lane reads of csrc/mlp_block_util.h
(row_ror:N: lane i of a 16-lane row reads lane (i - N) % 16; the permlane swaps pair lane i with i ^ 16 and
i ^ 32) and compares all 64 lanes bit for bit; rotating the other way (another association of the same four
addends) must not pass, so the comparison can tell the difference.  A second check runs the first level as
the kernels do, the lane's own product fused into the add.

The batch-size reciprocal: 1 / bs is evaluated once per launch for bs = B and per step only when bs != B."""
import numpy as np
import pytest

LANES = np.arange(64)


def _ror(v, n):
    """DPP row_ror:n on [..., 64] values: lane i reads lane (i - n) % 16 of its own 16-lane row."""
    src = (LANES & ~15) | ((LANES - n) & 15)
    return v[..., src]


def _xor(v, bit):
    return v[..., LANES ^ bit]


def _sum_bits2to5(v):
    """bku::sum_bits2to5: rotations by 4 and 8 inside the row, then the two permlane swap sums."""
    v = v + _ror(v, 4)
    v = v + _ror(v, 8)
    v = v + _xor(v, 16)
    return v + _xor(v, 32)


def _all_reduce_then_select(x0, x1):
    cb = ((LANES >> 2) & 1).astype(bool)
    return np.where(cb, _sum_bits2to5(x1), _sum_bits2to5(x0))


def _reduce_scatter(x0, x1, first_rotation=4):
    cb = ((LANES >> 2) & 1).astype(bool)
    keep, send = np.where(cb, x1, x0), np.where(cb, x0, x1)
    s = keep + _ror(send, first_rotation)
    s = s + _ror(s, 8)
    s = s + _xor(s, 16)
    return s + _xor(s, 32)


@pytest.fixture(scope="module")
def shares():
    """2,000 trials of both classes' per-lane products, magnitudes spread over many binades so that the
    association of the adds shows in the low bits; a few rows of signed zeros, denormals and infinities."""
    rng = np.random.default_rng(12)
    mag = np.exp2(rng.integers(-20, 21, size=(2, 2000, 64))).astype(np.float32)
    x = (rng.standard_normal((2, 2000, 64)).astype(np.float32) * mag).astype(np.float32)
    x[:, 0, :] = 0.0
    x[:, 1, ::2] = -0.0
    x[:, 2, :] = np.float32(1e-42)
    x[0, 3, 5] = np.inf
    x[1, 4, 9] = -np.inf
    return x[0], x[1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_logit_reduce_scatter_equals_all_reduce_bitwise(shares):
    x0, x1 = shares
    with np.errstate(invalid="ignore", over="ignore"):
        ref = _all_reduce_then_select(x0, x1)
        new = _reduce_scatter(x0, x1)
    assert ref.dtype == np.float32 and new.dtype == np.float32
    assert np.array_equal(_bits(ref), _bits(new))
    # the stored lanes 0..7 ([class][row]) hold both classes of all four rows
    cls, row = (LANES[:8] >> 2) & 1, LANES[:8] & 3
    assert sorted(zip(cls.tolist(), row.tolist())) == [(c, r) for c in range(2) for r in range(4)]


def test_logit_reduce_scatter_other_rotation_is_another_sum(shares):
    """row_ror:12 also delivers the right class (lane i + 4 has the opposite bit 2 too) but pairs the addends
    differently: same sums in exact arithmetic, other bits in float32 - the check above is not blind."""
    x0, x1 = shares
    with np.errstate(invalid="ignore", over="ignore"):
        ref = _all_reduce_then_select(x0[5:], x1[5:])
        other = _reduce_scatter(x0[5:], x1[5:], first_rotation=12)
        scale = _all_reduce_then_select(np.abs(x0[5:]), np.abs(x1[5:]))
    assert not np.array_equal(_bits(ref), _bits(other))
    assert np.all(np.abs(ref - other) <= 16 * np.float32(2.0 ** -23) * scale)  # the same 16 addends


def _fma(a, b, c):
    """fma of float32 operands: the product of two 24-bit significands is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def test_logit_reduce_scatter_equals_all_reduce_with_fused_first_level(shares):
    """The form the kernels run: sum_bits2to5(w * h2) compiles its first level to fma(w, h2, ror4(w * h2)) - the
    lane's own product fused, the neighbour's rounded.  The reduce-scatter spells the same out: the kept
    class's weight in the fma, the sent class's rounded product through the rotation."""
    w0, w1 = shares
    rng = np.random.default_rng(5)
    h2 = np.maximum(rng.standard_normal(w0.shape).astype(np.float32), 0)
    cb = ((LANES >> 2) & 1).astype(bool)

    def tail(v):
        v = v + _ror(v, 8)
        v = v + _xor(v, 16)
        return v + _xor(v, 32)

    with np.errstate(invalid="ignore", over="ignore"):
        t0 = tail(_fma(w0, h2, _ror(w0 * h2, 4)))
        t1 = tail(_fma(w1, h2, _ror(w1 * h2, 4)))
        ref = np.where(cb, t1, t0)
        wk, ws = np.where(cb, w1, w0), np.where(cb, w0, w1)
        new = tail(_fma(wk, h2, _ror(ws * h2, 4)))
        unfused = tail(wk * h2 + _ror(ws * h2, 4))
    assert np.array_equal(_bits(ref), _bits(new))
    assert not np.array_equal(_bits(ref[5:]), _bits(unfused[5:]))  # rounding the kept product first is visible


def _rcp(x):
    return np.float32(1.0) / np.float32(x)


def _inv_bs_per_step(bs):
    return _rcp(np.float32(bs if bs > 0 else 1))


def _inv_bs_hoisted(bs, B, launch_value):
    return launch_value if bs == B else _rcp(np.float32(bs if bs > 0 else 1))


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_inv_bs_select_matches_per_step_form(B):
    launch_value = _rcp(np.float32(B if B > 0 else 1))  # once per launch
    for bs in range(1, B + 1):  # a full batch, or a dataset's last one
        per_step = _inv_bs_per_step(bs)
        hoisted = _inv_bs_hoisted(bs, B, launch_value)
        assert _bits(per_step) == _bits(hoisted)
        # the row factor of the loss block and wave 0's batch loss take the same value
        tls = np.float32(1.2345678)
        assert _bits(tls * hoisted) == _bits(tls * _rcp(np.float32(bs)))
    for bs in (0, -3):  # steps past the dataset's end: no live row, the guarded operand is 1
        assert _bits(_inv_bs_hoisted(bs, B, launch_value)) == _bits(_inv_bs_per_step(bs)) == _bits(np.float32(1.0))
