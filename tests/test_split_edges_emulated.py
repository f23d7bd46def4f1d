"""The split-row producers and the split GEMM on the CPU (csrc/gemm_split.hip, csrc/norm.hip through tests/emu) at the
edges of the formats' value range (tests/split_edges.py, the same inputs as tests/test_gpu_split_edges.py): rounding
ties of every conversion, the exact thresholds of the overflow word, operands whose fp16 hi plane is subnormal, a
near-zero weight matrix through the x8 chain."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import build_emu  # noqa: E402

import split_edges as E  # noqa: E402
from text2human_amd._lib import GemmSplitArgs  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')


class Emulated:
    def __init__(self):
        self.gemm_lib = build_emu.load('gemm_split.hip')
        self.norm_lib = build_emu.load('norm.hip')

    @staticmethod
    def _out(rows, C):
        return torch.zeros((rows, C // 32, 2, 32), dtype=torch.int16), torch.zeros(1, dtype=torch.int32)

    def split_rows(self, x):
        out, ovf = self._out(*x.shape)
        rc = self.gemm_lib.t2h_split_rows_f32(x.data_ptr(), x.shape[1], out.data_ptr(), x.shape[0], x.shape[1], ovf.data_ptr(), None)
        assert rc == 0, self.gemm_lib.emu_last_error()
        return out, int(ovf[0])

    def split_rows_x8(self, x, s):
        out, ovf = self._out(*x.shape)
        rc = self.gemm_lib.t2h_split_rows_x8_f32(x.data_ptr(), x.shape[1], out.data_ptr(), x.shape[0], x.shape[1], s, ovf.data_ptr(), None)
        assert rc == 0, self.gemm_lib.emu_last_error()
        return out, int(ovf[0])

    def layernorm_split(self, x, g, b):
        out, ovf = self._out(*x.shape)
        rc = self.norm_lib.t2h_layernorm_split_f32(x.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                                   1e-5, ovf.data_ptr(), None)
        assert rc == 0, self.norm_lib.emu_last_error()
        return out, int(ovf[0])

    def layernorm_x8(self, x, g, b, s):
        out, ovf = self._out(*x.shape)
        rc = self.norm_lib.t2h_layernorm_x8_f32(x.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                                1e-5, s, ovf.data_ptr(), None)
        assert rc == 0, self.norm_lib.emu_last_error()
        return out, int(ovf[0])

    def gemm(self, A, B, M, N, K, x8=None, cfg=-1, out_split=None):
        lib = self.gemm_lib
        g = GemmSplitArgs()
        out = torch.full((M, N), float('nan'))
        ovf = torch.zeros(1, dtype=torch.int32)
        rows = None
        if x8 is not None:
            g.fmt, g.lo_mul = 1, 1.0 / (2048.0 * x8[0] * x8[1])
        g.A, g.B, g.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
        g.M, g.N, g.K, g.ldc = M, N, K, N
        if out_split is not None:
            rows = torch.zeros((M, N // 32, 2, 32), dtype=torch.int16)
            g.C_split, g.overflow_flag = rows.data_ptr(), ovf.data_ptr()
            if out_split != 'fp16':
                g.out_fmt, g.out_scale = 1, float(out_split)
        old = lib.t2h_gemm_split_force_config(cfg)
        try:
            assert cfg < 0 or lib.t2h_gemm_split_tile_config(ctypes.byref(g)) == cfg
            rc = lib.t2h_gemm_split_f32(ctypes.byref(g), None)
        finally:
            lib.t2h_gemm_split_force_config(old)
        assert rc == 0, lib.emu_last_error()
        return out, rows, int(ovf[0])


@pytest.fixture(scope='module')
def be():
    return Emulated()


def test_emulated_fp16_plane_rounding_ladder(be):
    E.ladder_fp16_planes(be)


def test_emulated_x8_rounding_ladder(be):
    E.ladder_x8_planes(be)


def test_emulated_overflow_thresholds_of_the_producers(be):
    E.thresholds_producers(be)


def test_emulated_overflow_thresholds_of_layernorm(be):
    E.thresholds_layernorm(be)


def test_emulated_overflow_thresholds_of_the_gemm_epilogue(be):
    E.thresholds_gemm_epilogue(be)


@pytest.mark.parametrize('both', [False, True], ids=['w-2e-5', 'a-and-w-2e-5'])
@pytest.mark.parametrize('x8', [False, True], ids=['fp16-planes', 'x8'])
@pytest.mark.parametrize('cfg,M,N,K', E.SUBNORMAL_SHAPES)
def test_emulated_gemm_on_subnormal_hi_planes(be, cfg, M, N, K, x8, both):
    E.gemm_on_subnormal_planes(be, cfg, M, N, K, x8, both)


def test_emulated_near_zero_weight_matrix_through_the_x8_chain(be):
    E.near_zero_weight_chain(be)
