"""Guard-band and image-border tests of the decode / encode kernels (-m gpu): the convolutional half of the library
between guard bands, as tests/test_gpu_row_counts.py holds the sampler's GEMM chain.  The property code is
tests/decode_bands.py (P1 accuracy, P2 untouched bands, P3 inputs in longer buffers = the image-border test, P4 the
range guard is not vacuous, P5 image independence: see there); every kernel is called through its C entry point
(text2human_amd._lib) with buffers of the test's own.  The CPU twin is tests/test_decode_bands_emulated.py.

Shapes: the smallest that still reach the edge, W != H everywhere.  Where an entry point rejects a listed shape the
nearest accepted one stands in, noted at the case."""
import pytest

import decode_bands as D
from text2human_amd import _lib, ops

pytestmark = pytest.mark.gpu

ENV = D.Env('cuda', lambda kernel_file: _lib.load(), ops._stream,
            lambda lib: (lib.t2h_last_error() or b'?').decode())
GEMM = dict(band_out=128, lda_extra=16, ldc_extra=24)   # lda = 48, ldc = 64 around cin = 32, cout = 40; 128-row tiles


# ---- t2h_gemm_f32, conv mode: cin = 32, cout = 40, 6 x 10, 3 images: M = 180 (60 for the image alone) is no multiple of
# a row tile, N = 40 a partial column tile; bias + residual


@pytest.mark.parametrize('pro', [False, True], ids=['plain', 'groupnorm-tables'])
@pytest.mark.parametrize('mode', ['same', 'up', 'down'])
def test_gemm_conv_borders_and_bands(mode, pro):
    p = D.conv_problem(3, 32, 40, 6, 10, mode, pro=pro)
    D.conv_case(ENV, 'gemm', p, pro_extra=16, **GEMM)


@pytest.mark.parametrize('cfg', [0, 1, 2, 3, 6])
@pytest.mark.parametrize('mode', ['same', 'down'])
def test_gemm_conv_forced_tile(mode, cfg):
    """every tile configuration the shape supports (Cin = 32: none of the K = 64 ones); the generic GroupNorm prologue
    (60 pixels per image are no multiple of a row tile) runs on 0 .. 3 only"""
    lib = _lib.load()
    with ENV.forced('gemm.hip', 't2h_gemm_force_config', cfg):
        for pro in ((False, True) if cfg <= 3 else (False, )):
            p = D.conv_problem(3, 32, 40, 6, 10, mode, pro=pro)
            D.conv_case(ENV, 'gemm', p, pro_extra=16, **GEMM)
    assert lib.t2h_gemm_force_config(-1) == -1


@pytest.mark.parametrize('h,w', [(2, 1), (4, 2)])
def test_gemm_conv_split_over_k_with_an_exact_workspace(h, w):
    """the deep UNet levels: cin = 512, cout = 96, 3 images; 2 and 3 slices forced, and the library's own choice -- the
    workspace exactly ksplit * M * N floats between bands; P5 bit for bit within one ksplit (the header's promise: the
    slice count never comes from the number of images).  A forced split equals the single pass within P1's bound."""
    p = D.conv_problem(3, 512, 96, h, w, 'same', seed=200)
    one = D.conv_case(ENV, 'gemm', p, band_out=128, ldc_extra=32, ksplit=1)['C'].view(D.F32).double()
    for ks in (2, 3, 0):
        got = D.conv_case(ENV, 'gemm', p, band_out=128, ldc_extra=32, ksplit=ks)['C'].view(D.F32).double()
        assert ((got - one).abs() <= 2e-5 + 2e-5 * p.ref.view_as(one).abs()).all()


def test_plain_gemm_into_the_right_half_of_a_wider_buffer():
    D.plain_gemm_into_the_right_half(ENV)


# ---- t2h_conv_split_f32: cin = 64, cout = 96, 3 images, 16 x 8 (128 pixels per image, the minimum) for the 128-row tile.
# The entry point rejects the 256-row tile below 256 pixels per image (so M is always whole tiles of it): it runs 32 x 8.


@pytest.mark.parametrize('res_pre', [0, 1])
@pytest.mark.parametrize('taps', [9, 1])
@pytest.mark.parametrize('mode', ['same', 'up'])
@pytest.mark.parametrize('tile', [128, 256])
def test_conv_split_borders_and_bands(tile, mode, taps, res_pre):
    h, w = (16, 8) if tile == 128 else (32, 8)
    if mode == 'up':
        h, w = h // 2, w // 2
    p = D.conv_problem(3, 64, 96, h, w, mode, taps=taps, res_pre=res_pre, seed=400)
    with ENV.forced('conv_split.hip', 't2h_conv_split_force_tile', tile):
        D.conv_case(ENV, 'split', p, band_out=256, ldc_extra=32, gn_stats=True)


# ---- t2h_conv_halo_f32: 16 x 32 output, 3 images; cin = 32 / cout = 96 and cin = 96 (an odd number of channel groups) /
# cout = 136 (one full and one 8-wide column tile); lda = cin + 32, ldc = cout + 32, band = 16 * Wout rows


@pytest.mark.parametrize('pro', [False, True], ids=['plain', 'groupnorm-tables'])
@pytest.mark.parametrize('cin,cout', [(32, 96), (96, 136)])
@pytest.mark.parametrize('mode', ['same', 'up'])
@pytest.mark.parametrize('variant', [1, 0], ids=['lds-dma-kernel', 'first-version'])
def test_conv_halo_borders_bands_and_range_guard(variant, mode, cin, cout, pro):
    h, w = (16, 32) if mode == 'same' else (8, 16)
    p = D.conv_problem(3, cin, cout, h, w, mode, pro=pro, seed=500)
    with ENV.forced('conv_halo.hip', 't2h_conv_halo_force_variant', variant):
        D.conv_case(ENV, 'halo', p, p4=True, band_out=16 * p.wo, lda_extra=32, ldc_extra=32, pro_extra=32, gn_stats=True)


# ---- GroupNorm, conv_out, AttnBlock attention


def test_gn_apply_split_columns_range_guard_and_images():
    D.gn_apply_split_case(ENV)


def test_groupnorm_tables_and_finalize_between_bands():
    D.groupnorm_tables_case(ENV)
    D.groupnorm_finalize_case(ENV)


@pytest.mark.parametrize('pro', [False, True], ids=['plain', 'groupnorm-tables'])
@pytest.mark.parametrize('cout', [3, 4])
def test_conv_small_borders_and_strided_output(cout, pro):
    D.conv_small_case(ENV, cout, pro)


def test_spatial_attention_between_bands():
    D.spatial_attention_case(ENV)


# ---- quantizers and layout kernels


def test_vq_index_lists_between_bands():
    D.vq_l2_argmin_case(ENV)
    D.vq_argmin_tex_case(ENV, fold=False)
    D.vq_argmin_tex_case(ENV, fold=True)
    D.codebook_gathers_case(ENV)
    D.routed_head_argmax_case(ENV)


def test_layout_kernels_between_bands():
    D.layout_cases(ENV)

