"""Guard-band and image-border tests of the decode / encode kernels on the CPU: the CPU twin of
tests/test_gpu_decode_bands.py.  The property code is tests/decode_bands.py (P1 .. P5, see there); here every kernel
runs from its SOURCE through tests/emu on host tensors, so the bands live in host memory and P2 (untouched bands) is
exact.  Every kernel at its smallest listed shape; the emulator runs workgroups one after the other on OS threads, so
the forced tile configurations, the second split-K geometry and the full mode x tile x taps products stay with the
GPU file."""
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import build_emu  # noqa: E402
import decode_bands as D  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')


@functools.lru_cache(maxsize=None)
def _load(kernel_file):
    return build_emu.load(kernel_file)


ENV = D.Env('cpu', _load, lambda: None, lambda lib: lib.emu_last_error())


# ---- t2h_gemm_f32, conv mode: cin = 32, cout = 40, 6 x 10, 3 images: M = 180 (60 for the image alone) is no multiple of
# a row tile, N = 40 a partial column tile; lda = 48, ldc = 64, bias + residual


@pytest.mark.parametrize('mode,pro', [('up', False), ('down', False), ('same', True)])
def test_emulated_gemm_conv_borders_and_bands(mode, pro):
    p = D.conv_problem(3, 32, 40, 6, 10, mode, pro=pro)
    D.conv_case(ENV, 'gemm', p, band_out=128, lda_extra=16, ldc_extra=24, pro_extra=16)


@pytest.mark.parametrize('cfg', [3])
def test_emulated_gemm_conv_forced_tile(cfg):
    """the 128 x 128 tile (the automatic choice above is 128 x 64 for the batch, 64 x 64 for the image alone)"""
    p = D.conv_problem(3, 32, 40, 6, 10, 'same')
    with ENV.forced('gemm.hip', 't2h_gemm_force_config', cfg):
        D.conv_case(ENV, 'gemm', p, band_out=128, lda_extra=16, ldc_extra=24)


def test_emulated_gemm_conv_split_over_k_with_an_exact_workspace():
    """cout = 96, 2 x 1, 3 images, cin = 128 (the GPU file runs the deep levels' 512: four times the K loop, and the
    emulator pays for every barrier of it): 2 slices forced, and the library's own choice (9); the workspace is
    exactly ksplit * M * N floats between bands.  A forced split equals the single pass within P1's bound."""
    p = D.conv_problem(3, 128, 96, 2, 1, 'same', seed=200)
    kw = dict(band_out=128, ldc_extra=32)
    one = D.conv_run(ENV, 'gemm', p, ksplit=1, **kw)((0, 1, 2), False)['C'].view(D.F32).double()
    for ks, p5 in ((2, True), (0, False)):
        got = D.conv_case(ENV, 'gemm', p, p5=p5, ksplit=ks, **kw)['C'].view(D.F32).double()
        assert ((got - one).abs() <= 2e-5 + 2e-5 * p.ref.view_as(one).abs()).all()


def test_emulated_plain_gemm_into_the_right_half_of_a_wider_buffer():
    D.plain_gemm_into_the_right_half(ENV)


# ---- t2h_conv_split_f32: cin = 64, cout = 96, 16 x 8 (128 pixels per image, the minimum) for the 128-row tile; the
# 256-row tile is rejected below 256 pixels per image, so it runs 32 x 8 -- ldc = 128, gn_part_out banded


@pytest.mark.parametrize('tile,mode,taps,res_pre', [(128, 'same', 9, 0), (128, 'up', 9, 1), (256, 'up', 1, 1)])
def test_emulated_conv_split_borders_and_bands(tile, mode, taps, res_pre):
    h, w = (16, 8) if tile == 128 else (32, 8)
    if mode == 'up':
        h, w = h // 2, w // 2
    p = D.conv_problem(3, 64, 96, h, w, mode, taps=taps, res_pre=res_pre, seed=400)
    with ENV.forced('conv_split.hip', 't2h_conv_split_force_tile', tile):
        D.conv_case(ENV, 'split', p, band_out=256, ldc_extra=32, gn_stats=True)


# ---- t2h_conv_halo_f32 at cin = 32, cout = 96, 16 x 32, 3 images: one case of the LDS-DMA kernel (tables), one of the first
# kernel (nearest x2, no tables); lda = cin + 32, ldc = cout + 32, band = 16 * Wout rows.  (cin = 96 / cout = 136 -- an odd
# number of channel groups, an 8-wide column tile -- takes the emulator a minute per case: GPU file)


@pytest.mark.parametrize('variant,cin,cout,mode,pro', [(1, 32, 96, 'same', True), (0, 32, 96, 'up', False)])
def test_emulated_conv_halo_borders_bands_and_range_guard(variant, cin, cout, mode, pro):
    h, w = (16, 32) if mode == 'same' else (8, 16)
    p = D.conv_problem(3, cin, cout, h, w, mode, pro=pro, seed=500)
    with ENV.forced('conv_halo.hip', 't2h_conv_halo_force_variant', variant):
        D.conv_case(ENV, 'halo', p, p4=True, band_out=16 * p.wo, lda_extra=32, ldc_extra=32, pro_extra=32, gn_stats=True)


# ---- GroupNorm, conv_out, AttnBlock attention


def test_emulated_gn_apply_split_columns_range_guard_and_images():
    D.gn_apply_split_case(ENV)


def test_emulated_groupnorm_tables_and_finalize_between_bands():
    D.groupnorm_tables_case(ENV)
    D.groupnorm_finalize_case(ENV)


@pytest.mark.parametrize('cout,pro', [(3, True), (4, False)])
def test_emulated_conv_small_borders_and_strided_output(cout, pro):
    D.conv_small_case(ENV, cout, pro)


def test_emulated_spatial_attention_between_bands():
    D.spatial_attention_case(ENV)


# ---- quantizers and layout kernels


def test_emulated_vq_index_lists_between_bands():
    """(the texture-routed argmin and the routed head run 37 rows and 13 codes here, 111 and 37 on the GPU: one wave per
    row and two wave-wide sums per code are what the emulator is slowest at)"""
    D.vq_l2_argmin_case(ENV)
    D.vq_argmin_tex_case(ENV, fold=False, n=37, n_e=13)
    D.vq_argmin_tex_case(ENV, fold=True, n=37, n_e=13)
    D.codebook_gathers_case(ENV)
    D.routed_head_argmax_case(ENV, n=37)


def test_emulated_layout_kernels_between_bands():
    D.layout_cases(ENV)
