"""mlp_block5's integer dropout keep test (b5_drop_int, csrc/mlp_block5_impl.h): the kernel drops an element
when ``(h >> 8) < ceil(p * 2^24)`` instead of ``u01(h) = (h >> 8) * 2^-24 < p``.  Both sides depend on the hash
only through its 24 high bits, so the equivalence is checked over every one of the 2^24 values, in the
kernel's fp32 arithmetic.  The host mirrors of the masks (ops/fused_mlp.py) keep the float compare and are
pinned to what they returned before."""
import zlib

import numpy as np
import pytest

import dct_amd  # noqa: F401
from dct_amd.ops.fused_mlp import dropout_keep_mask, wave_dropout_keep_mask

P_VALUES = [0.0, 3e-8, 1e-7, 0.1, 0.2, 1.0 / 3.0, 0.5, 1.0 - 2.0 ** -24, 1.0]


@pytest.fixture(scope="module")
def all_k():
    return np.arange(1 << 24, dtype=np.uint32)


@pytest.mark.parametrize("p", P_VALUES, ids=[repr(p) for p in P_VALUES])
def test_integer_threshold_equals_float_compare_for_every_hash(p, all_k):
    pf = np.float32(p)
    dropped_float = all_k.astype(np.float32) * np.float32(1.0 / 16777216.0) < pf  # u01(h) < p
    thr = np.uint32(np.ceil(pf * np.float32(16777216.0)))  # b5_drop_thr
    assert float(thr) >= float(pf) * 16777216.0 > float(thr) - 1  # the ceiling, p * 2^24 exact in fp32
    dropped_int = all_k < thr
    assert np.array_equal(dropped_float, dropped_int)
    if p in (0.0, 1.0):
        assert bool(dropped_int.all()) == (p == 1.0) and bool(dropped_int.any()) == (p == 1.0)
    if p == 3e-8:
        assert thr == 1  # p * 2^24 = 0.503: only h >> 8 == 0 is dropped
    if p == 1e-7:
        assert thr == 2


# (seed, gstep, layer, rows, units, p) -> (kept, crc32 of the packed mask)
PINS = {
    dropout_keep_mask: {(3, 0, 0, 4, 128, 0.2): (414, 1749797393),
                        (3, 69, 1, 4, 128, 0.2): (416, 2093480538),
                        (11, 12345, 1, 4, 128, 0.5): (273, 3982978614),
                        (7, 5, 0, 4, 64, 1e-7): (256, 4285311755),
                        (7, 5, 0, 4, 64, 0.0): (256, 4285311755),
                        (7, 5, 1, 4, 64, 1.0): (0, 420107693)},
    wave_dropout_keep_mask: {(3, 0, 0, 4, 128, 0.2): (402, 2274509589),
                             (3, 69, 1, 4, 128, 0.2): (439, 3258970481),
                             (11, 12345, 1, 4, 128, 0.5): (262, 1268817889),
                             (7, 5, 0, 4, 64, 1e-7): (256, 4285311755),
                             (7, 5, 0, 4, 64, 0.0): (256, 4285311755),
                             (7, 5, 1, 4, 64, 1.0): (0, 420107693)},
}


@pytest.mark.parametrize("fn", list(PINS), ids=[f.__name__ for f in PINS])
def test_host_mask_mirrors_unchanged(fn):
    for args, (kept, crc) in PINS[fn].items():
        m = fn(*args).numpy()
        assert m.shape == (args[3], args[4]) and m.dtype == np.bool_
        assert (int(m.sum()), zlib.crc32(np.packbits(m).tobytes())) == (kept, crc), args
