"""Host side of the batch-tiled fused trainer (csrc/mlp_tile.hip): the supported() mirror and the
dropout-mask mirror.  No GPU."""
import pytest
import torch

import dct_amd  # noqa: F401
from dct_amd.ops.fused_mlp import FusedMLPKernel, dropout_keep_mask

WEATHER = [5, 64, 2]
WEATHER_3X128 = [5, 128, 128, 2]


@pytest.mark.parametrize("dims", [WEATHER, WEATHER_3X128, [7, 48, 32, 3], [32, 128, 128, 4], [1, 16, 2]])
def test_supported_above_batch_16(dims):
    for batch in (17, 32, 1024):
        assert FusedMLPKernel.supported(dims, batch), (dims, batch)
    assert not FusedMLPKernel.supported(dims, 1025)


@pytest.mark.parametrize("dims", [[5, 72, 2], [40, 64, 2], [5, 64, 5], [5, 64, 64, 64, 2], [5, 144, 2], [5, 8, 2],
                                  [5, 64, 1]])
def test_unsupported_shapes_at_batch_64(dims):
    assert not FusedMLPKernel.supported(dims, 64)


# answers of the parent commit at batch <= 16 (the LDS / block / wave plans): unchanged
_SMALL = [([5, 64, 2], True), ([5, 128, 128, 2], True), ([5, 72, 2], True), ([40, 64, 2], True), ([5, 64, 5], True),
          ([16, 32, 48, 32, 3], True), ([5, 64, 64, 64, 64, 2], False), ([256, 1024, 1024, 1024, 2], False),
          ([5, 2], False)]


@pytest.mark.parametrize("dims,want", _SMALL)
def test_supported_at_small_batch_unchanged_and_tile_range_opens(dims, want):
    for batch in (1, 4, 5, 16):
        assert FusedMLPKernel.supported(dims, batch) == want, (dims, batch)
    assert not FusedMLPKernel.supported(dims, 0)
    # the headline models reach past batch 16 now (False on the parent)
    assert FusedMLPKernel.supported(WEATHER, 17) and FusedMLPKernel.supported(WEATHER_3X128, 256)


def test_dropout_keep_mask_shape_rate_and_keys():
    m = dropout_keep_mask(11, 3, 0, 100, 128, 0.2)
    assert m.shape == (100, 128) and m.dtype == torch.bool
    assert dropout_keep_mask(11, 3, 0, 100, 128, 0.0).all()
    kept = sum(int(dropout_keep_mask(7, s, 1, 64, 128, 0.2).sum()) for s in range(50))
    assert 0.78 < kept / (64 * 128 * 50) < 0.82
    big = dropout_keep_mask(11, 3, 0, 128, 128, 0.2)
    assert not torch.equal(big[0], big[64])
    assert torch.equal(big[:100], m)
    assert torch.equal(dropout_keep_mask(11, 3, 0, 100, 128, 0.2), m)
    # layer and step are part of the key
    assert not torch.equal(dropout_keep_mask(11, 3, 1, 100, 128, 0.2), m)
    assert not torch.equal(dropout_keep_mask(11, 4, 0, 100, 128, 0.2), m)


def test_dropout_keep_mask_matches_scalar_hash():
    """The vectorised mirror against a plain-int transcription of mix_hash / u01 (mlp_fused_impl.h)."""
    M = 0xFFFFFFFF

    def mix(a, b, c):
        h = (a * 0x9E3779B1) & M
        h ^= ((b + 0x7F4A7C15) * 0x85EBCA77) & M
        h ^= ((c + 0x165667B1) * 0xC2B2AE3D) & M
        h ^= h >> 16
        h = (h * 0x7FEB352D) & M
        h ^= h >> 15
        h = (h * 0x846CA68B) & M
        h ^= h >> 16
        return h

    seed, gstep, layer, p = 0xDEADBEEF, 12345, 1, 0.2
    m = dropout_keep_mask(seed, gstep, layer, 130, 40, p)
    p32 = float(torch.tensor(p, dtype=torch.float32))
    for b in (0, 1, 63, 64, 65, 129):
        for o in (0, 17, 39):
            h = mix((seed + (b >> 6) * 0x9E3779B9) & M, gstep, ((layer * 64 + (b & 63)) * 65536 + o) & M)
            assert bool(m[b, o]) == (not ((h >> 8) / 16777216.0 < p32)), (b, o)
