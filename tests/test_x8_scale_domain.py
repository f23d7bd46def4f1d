"""The domain of an x8 tensor's scale (host only): ops.x8_scale_for stays inside [2^-7, 2^22], and with its scale both
8-bit planes of any fp32 tensor stay inside e4m3's range -- computed here WITHOUT clamping.  The producers' range test
looks at |x| s alone; that bounds the residual plane only where the fp16 hi plane is a normal number (|l| <= |h|).  Where
it is subnormal, |l| reaches 2^-14 whatever |x| is: a scale of 2^23 and more (a tensor whose maximum is below 3e-5) put
l s beyond 448 with the overflow word at 0.  The wrappers that take a scale refuse one above 2^22 before any launch."""
import pytest
import torch

from text2human_amd import ops


def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


MAGNITUDES = [1e-8, 3e-8, 5.9e-8, 8.5e-7, 1e-6, 2.9e-6, 3.8e-6, 1.4e-5, 3.05e-5, 6.1e-5, 1e-4, 1e-3, 0.02, 1.0, 31.9, 32.0, 300.0, 1e4]


@pytest.mark.parametrize('target', [32.0, 256.0])
@pytest.mark.parametrize('mag', MAGNITUDES)
def test_both_8_bit_planes_stay_in_range_under_the_scale_of_the_maximum(mag, target):
    x = _rnd(64, 256, seed=3)
    x = x * (mag / float(x.abs().max()))          # max |x| = mag: all-subnormal fp16 planes below 6.1e-5, all-zero ones below 3e-8
    s = ops.x8_scale_for(x.abs().max(), target)
    assert 2.0 ** -7 <= s <= 2.0 ** 22
    h = x.half().float()
    l = (x - h) * ops.SPLIT_LO_SCALE
    assert torch.isfinite(h).all()
    assert float((h * s).abs().max()) <= 448.0
    assert float((l * s).abs().max()) < 448.0, (mag, target, s, float((l * s).abs().max()))
    if s < 2.0 ** 22 and s > 2.0 ** -7:           # (an unclamped scale puts the maximum where it is meant to be)
        assert target / 2 <= float(x.abs().max()) * s < target


@pytest.mark.parametrize('target', [32.0, 256.0])
def test_scale_of_zero_subnormal_and_non_finite_maxima(target):
    assert ops.x8_scale_for(0.0, target) == 1.0 and ops.x8_scale_for(float('nan'), target) == 1.0
    assert ops.x8_scale_for(float('inf'), target) == 1.0
    assert ops.x8_scale_for(torch.zeros(4, 32).abs().max(), target) == 1.0
    assert ops.x8_scale_for(1e-45, target) == 2.0 ** 22 and ops.x8_scale_for(1e-30, target) == 2.0 ** 22
    assert ops.x8_scale_for(1e30, target) == 2.0 ** -7


def test_scale_for_keeps_its_values_inside_the_domain():
    # (tests/test_gpu_x8.py's own assertions)
    assert ops.x8_scale_for(1.0) == 16.0 and ops.x8_scale_for(31.9) == 1.0 and ops.x8_scale_for(32.0) == 0.5 and ops.x8_scale_for(0.02, 256.0) == 8192.0
    assert ops.x8_scale_for(1.0e5) == 2.0 ** -7 and 448.0 / ops.x8_scale_for(1.0e9) < 65504.0
    # the last uncapped scales and the first capped ones
    assert ops.x8_scale_for(3.1e-5, 256.0) == 2.0 ** 22 and ops.x8_scale_for(6.2e-5, 256.0) == 2.0 ** 21
    assert ops.x8_scale_for(3.0e-5, 256.0) == 2.0 ** 22 and ops.x8_scale_for(1e-6, 256.0) == 2.0 ** 22
    assert ops.x8_scale_for(3.9e-6) == 2.0 ** 22 and ops.x8_scale_for(3.7e-6) == 2.0 ** 22 and ops.x8_scale_for(7.7e-6) == 2.0 ** 21
    assert ops.X8_SCALE_MIN == 2.0 ** -7 and ops.X8_SCALE_MAX == 2.0 ** 22


@pytest.mark.parametrize('scale', [2.0 ** 23, 2.0 ** 27, float('inf'), float('nan')])
def test_wrappers_refuse_a_scale_above_the_domain_before_any_launch(scale):
    """(host tensors and None operands: a call that got as far as the library would fail otherwise)"""
    x, g = torch.zeros(2, 256), torch.zeros(256)
    with pytest.raises(ValueError, match='2\\^22'):
        ops.split_rows_x8(x, scale)
    with pytest.raises(ValueError, match='2\\^22'):
        ops.layernorm_x8(x, g, g, None, scale)
    with pytest.raises(ValueError, match='2\\^22'):
        ops.mha_split_x8(None, 128, None, 1, 128, 1, None, scale)
    with pytest.raises(ValueError, match='2\\^22'):
        ops.gemm_split(None, None, 2, 256, 32, out_split=None, out_x8_scale=scale)
