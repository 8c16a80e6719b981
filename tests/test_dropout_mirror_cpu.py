"""Host mirrors of the fused trainers' dropout masks (ops/fused_mlp.py): ``dropout_keep_mask`` (mix_hash,
csrc/mlp_fused_impl.h: LDS, block and tile trainers), ``wave_dropout_keep_mask`` (wave_hash,
csrc/mlp_wave_impl.h: the single-wave and row-parallel kernels) and ``FusedMLPKernel.dropout_mask``,
which picks the family by the launcher's rule.  No GPU."""
import math

import pytest
import torch

import dct_amd  # noqa: F401
from dct_amd.ops import _native
from dct_amd.ops.fused_mlp import FusedMLPKernel, dropout_keep_mask, wave_dropout_keep_mask, wave_supported

M = 0xFFFFFFFF


def _p32(p):
    return float(torch.tensor(p, dtype=torch.float32))


def _scalar_mix_keep(seed, gstep, layer, b, o, p):
    """Plain-int transcription of mix_hash / u01 and the tile trainer's row fold."""
    a, c = (seed + (b >> 6) * 0x9E3779B9) & M, ((layer * 64 + (b & 63)) * 65536 + o) & M
    h = (a * 0x9E3779B1) & M
    h ^= ((gstep + 0x7F4A7C15) * 0x85EBCA77) & M
    h ^= ((c + 0x165667B1) * 0xC2B2AE3D) & M
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M
    h ^= h >> 15
    h = (h * 0x846CA68B) & M
    h ^= h >> 16
    return not ((h >> 8) / 16777216.0 < _p32(p))


def _scalar_wave_keep(seed, gstep, layer, b, j, p):
    """Plain-int transcription of the wave kernels' key, wave_hash and integer threshold."""
    hkey = ((seed * 0x9E3779B1) & M) ^ ((gstep * 0x85EBCA77) & M)
    k = hkey ^ (((layer * 4096 + b * 64 + j) * 0xC2B2AE3D) & M)
    k ^= k >> 16
    k = (k * 0x7FEB352D) & M
    k ^= k >> 15
    k = (k * 0x846CA68B) & M
    k ^= k >> 16
    return not (k < int(_p32(p) * 4294967296.0))


MIRRORS = [(dropout_keep_mask, _scalar_mix_keep, 130), (wave_dropout_keep_mask, _scalar_wave_keep, 8)]


@pytest.mark.parametrize("mirror,scalar,rows", MIRRORS)
@pytest.mark.parametrize("seed,gstep,layer,p", [(0xDEADBEEF, 12345, 1, 0.2), (11, 5, 0, 0.2), (0, 0, 0, 0.5),
                                                (0xFFFFFFFF, 0xFFFFFFFE, 1, 0.73)])
def test_mirror_matches_scalar_hash(mirror, scalar, rows, seed, gstep, layer, p):
    m = mirror(seed, gstep, layer, rows, 64, p)
    assert m.shape == (rows, 64) and m.dtype == torch.bool
    for b in range(rows):
        for o in range(64):
            assert bool(m[b, o]) == scalar(seed, gstep, layer, b, o, p), (b, o)


@pytest.mark.parametrize("mirror", [dropout_keep_mask, wave_dropout_keep_mask])
def test_keep_rate_within_binomial_band(mirror):
    p, steps, rows, units = 0.2, 60, 8, 64
    for layer in (0, 1):
        kept = sum(int(mirror(7, s, layer, rows, units, p).sum()) for s in range(steps))
        n = steps * rows * units
        band = 5.0 * math.sqrt(p * (1 - p) / n)
        print("%s layer %d keep rate %.5f (band %.5f)" % (mirror.__name__, layer, kept / n, band))
        assert abs(kept / n - (1 - p)) < band


@pytest.mark.parametrize("mirror", [dropout_keep_mask, wave_dropout_keep_mask])
def test_p_zero_keeps_everything(mirror):
    for s in range(8):
        assert mirror(0x1234567, s, s & 1, 8, 64, 0.0).all()


@pytest.mark.parametrize("mirror", [dropout_keep_mask, wave_dropout_keep_mask])
def test_mask_depends_on_seed_step_layer_and_row(mirror):
    base = mirror(11, 5, 0, 8, 64, 0.2)
    assert torch.equal(mirror(11, 5, 0, 8, 64, 0.2), base)
    assert not torch.equal(mirror(12, 5, 0, 8, 64, 0.2), base)
    assert not torch.equal(mirror(11, 6, 0, 8, 64, 0.2), base)
    assert not torch.equal(mirror(11, 5, 1, 8, 64, 0.2), base)
    for b in range(8):
        for c in range(b):
            assert not torch.equal(base[b], base[c]), (b, c)
    # a smaller batch draws the first rows of the larger one (the key holds the row, not the batch)
    assert torch.equal(mirror(11, 5, 0, 3, 64, 0.2), base[:3])
    assert torch.equal(mirror(11, 5, 0, 8, 20, 0.2), base[:, :20])


def test_the_two_families_differ():
    assert not torch.equal(dropout_keep_mask(11, 5, 0, 8, 64, 0.2), wave_dropout_keep_mask(11, 5, 0, 8, 64, 0.2))


# (dims, batch) -> the wave kernels take it (csrc/mlp_wave.hip dct_mlp_wave_supported)
WAVE_CASES = [([5, 64, 2], 1, True), ([5, 64, 2], 8, True), ([5, 64, 2], 9, False), ([5, 64, 2], 16, False),
              ([16, 64, 4], 5, True), ([17, 64, 4], 5, False), ([16, 65, 4], 5, False), ([16, 64, 5], 5, False),
              ([9, 48, 64, 3], 8, True), ([9, 48, 64, 3], 9, False), ([9, 48, 72, 3], 4, False),
              ([12, 40, 40, 4], 6, True), ([5, 128, 128, 2], 4, False), ([5, 32, 32, 32, 2], 4, False),
              ([7, 20, 2], 8, True), ([7, 20, 2], 9, False)]


@pytest.mark.parametrize("dims,batch,want", WAVE_CASES)
def test_wave_supported_mirror(dims, batch, want):
    assert wave_supported(dims, batch) == want


def test_wave_supported_refuses_an_empty_batch():
    assert not wave_supported([5, 64, 2], 0) and not wave_supported([9, 48, 64, 3], 0)


@pytest.fixture
def nat(monkeypatch):
    """The native extension's plan is host code: a build or import failure fails these tests."""
    for k in ("DCT_MLP_KERNEL", "DCT_MLP_BLOCK"):
        monkeypatch.delenv(k, raising=False)
    n = _native.native()
    n.reload_knobs()
    yield n
    monkeypatch.undo()
    n.reload_knobs()


@pytest.mark.parametrize("dims,batch,want", WAVE_CASES)
def test_dropout_mask_picks_the_launchers_family(dims, batch, want, nat):
    k = FusedMLPKernel(dims, bmax=4 if batch <= 4 else 16)
    assert bool(k.plan.use_wave) == wave_supported(dims, 1)
    for layer in range(len(dims) - 2):
        mirror = wave_dropout_keep_mask if want else dropout_keep_mask
        got = k.dropout_mask(11, 5, layer, batch, 0.2)
        assert got.shape == (batch, dims[layer + 1])
        assert torch.equal(got, mirror(11, 5, layer, batch, dims[layer + 1], 0.2))
    with pytest.raises(ValueError):
        k.dropout_mask(11, 5, len(dims) - 2, batch, 0.2)


def test_dropout_mask_follows_the_plans_knobs(nat, monkeypatch):
    """DCT_MLP_KERNEL=lds takes a wave-shaped net to the LDS trainer, and the tile plan (batch > 16) never
    draws the wave mask."""
    want = dropout_keep_mask(11, 5, 0, 6, 40, 0.2)
    assert torch.equal(FusedMLPKernel([12, 40, 4], bmax=16).dropout_mask(11, 5, 0, 6, 0.2),
                       wave_dropout_keep_mask(11, 5, 0, 6, 40, 0.2))
    monkeypatch.setenv("DCT_MLP_KERNEL", "lds")
    k = FusedMLPKernel([12, 40, 4], bmax=16)
    assert not k.plan.use_wave
    assert torch.equal(k.dropout_mask(11, 5, 0, 6, 0.2), want)
    monkeypatch.delenv("DCT_MLP_KERNEL")
    k = FusedMLPKernel([5, 64, 2], bmax=1024)
    assert k.plan.use_tile and not k.plan.use_wave
    assert torch.equal(k.dropout_mask(11, 5, 0, 100, 0.2), dropout_keep_mask(11, 5, 0, 100, 64, 0.2))
    assert torch.equal(k.dropout_mask(11, 5, 0, 8, 0.2), dropout_keep_mask(11, 5, 0, 8, 64, 0.2))
