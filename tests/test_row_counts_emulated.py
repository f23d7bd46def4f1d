"""The split GEMM and the row producers at row counts that are NOT a multiple of the tile, inside LONGER buffers, on
the CPU (csrc/gemm_split.hip, norm.hip, misc.hip through tests/emu): what the sampler's rounds run
(engine.SamplerNet.finish_tail: m = 1..256 rows of buffers that hold 256, the rows behind m stale).  Four properties
for every case (tests/guard_util.py; host memory makes the band comparison exact):

  P1  accuracy against a reference of the same operation (the bounds of tests/test_gpu_split.py / test_gpu_x8.py);
  P2  every output sits between guard bands that are byte-identical after the launch;
  P3  every input the product keeps in a longer buffer sits between bands too: zero bands and poisoned bands give
      bitwise-equal outputs and leave the sticky overflow word 0;
  P4  the same launch with ONE out-of-range value inside the extent (row M - 1, last column) raises the overflow bit,
      so P3's zero is not vacuous.

Host memory makes P2 exact here.  Not covered here: the tiled kernel's x8 split-row STORE on a partial row tile (see
GemmCase), tile configurations 8 / 10 (256- and 128 x 192 tiles: too many OS threads per case) and attention."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import build_emu  # noqa: E402
import guard_util as G  # noqa: E402
from split_ref import emulate_x8, x8_planes_host, x8_rows_host  # noqa: E402

from text2human_amd import ops  # noqa: E402
from text2human_amd._lib import GemmSplitArgs  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')

VALID_ROW = 3   # what the index list holds behind n_rows and in its bands: a row that exists
BAND = 128   # rows: a whole 128-row tile fits behind the smallest extent, so an unmasked tile store lands in the band


@pytest.fixture(scope='module', params=[0, 1], ids=['requests-land-at-issue', 'requests-land-at-the-wait'])
def lib(request):
    so = build_emu.load('gemm_split.hip')
    so.emu_set_deferred(request.param)
    yield so
    so.emu_set_deferred(0)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def f32_poison(whole):
    """rows alternate between the NaN pattern (invisible to a `>=` range guard, fatal in a sum) and 1e30 (visible)"""
    G.fill_bits(whole, G.F32_NAN)
    G.bits(whole)[1::2] = G.F32_BIG


def rows_poison(x8):
    return G.x8_poison() if x8 else G.SPLIT_INF


class GemmCase:
    """C[M, N] (fp32, leading dimension N + 16, residual in place) and its split-row form from one launch, operands
    drawn like tests/test_gpu_x8.py.  x8_out: the split-row output in the x8 format -- here only with the few-rows
    kernel: the tiled kernel's x8 store swaps halves between lane pairs by DPP AFTER the lanes of masked rows have
    left, which the hardware allows and the emulator's wave-collective lane exchange does not (it would wait for the
    lanes that left)."""
    LD_EXTRA, C0 = 16, 8

    def __init__(self, M, N, K, x8, x8_out):
        self.M, self.N, self.K, self.x8, self.x8_out = M, N, K, x8, x8_out
        self.a, self.w = rnd(M, K, seed=31) * 1.3, rnd(N, K, seed=32, scale=0.07)
        self.bias, self.res = rnd(N, seed=33), rnd(M, N, seed=34)
        if x8:
            self.sa, self.sw = ops.x8_scale_for(float(self.a.abs().max())), ops.x8_scale_for(float(self.w.abs().max()), 256.0)
            assert float(self.a.abs().max()) * self.sa < 448.0 and float(self.w.abs().max()) * self.sw < 448.0
            self.A, self.B = x8_rows_host(self.a, self.sa), x8_rows_host(self.w, self.sw)
            self.lin = emulate_x8(self.a, self.w, self.sa, self.sw) + self.bias.double()
            self.ref = self.lin + self.res.double()
        else:
            self.A, self.B = ops.pack_split_rows_host(self.a), ops.pack_split_rows_host(self.w)
            self.lin = self.a.double() @ self.w.double().t() + self.bias.double()
            self.ref = self.lin + self.res.double()
        assert float(self.ref.abs().max()) < 65504.0
        if x8_out:
            self.so = ops.x8_scale_for(float(self.ref.abs().max()))
            assert float(self.ref.abs().max()) * self.so < 448.0     # the reference alone stays in range
        self.scale = self.a.double().abs() @ self.w.double().abs().t()

    def launch(self, lib, cfg, poison, res=None):
        """-> (C bits, split-row bits, overflow word); P2 is asserted here for both outputs"""
        M, N, K, x8 = self.M, self.N, self.K, self.x8
        ldc = N + self.LD_EXTRA
        a_whole, a_view = G.banded(M, (K // 32, 2, 32), torch.int16, 'cpu', BAND, rows_poison(x8) if poison else 0)
        a_view.copy_(self.A)
        c_whole, c_rows = G.banded(M, (ldc, ), torch.float32, 'cpu', BAND, f32_poison if poison else 0)
        if poison:
            f32_poison(c_rows)                      # (the columns beside the extent too)
        c_view = c_rows[:, self.C0:self.C0 + N]
        c_view.copy_(self.res if res is None else res)
        s_whole, s_view = G.banded(M, (N // 32, 2, 32), torch.int16, 'cpu', BAND, rows_poison(self.x8_out) if poison else 0)
        s_view.zero_()
        ovf = torch.zeros(1, dtype=torch.int32)
        g = GemmSplitArgs()
        if x8:
            g.fmt, g.lo_mul = 1, 1.0 / (ops.SPLIT_LO_SCALE * self.sa * self.sw)
        if self.x8_out:
            g.out_fmt, g.out_scale = 1, self.so
        g.A, g.B, g.bias = a_view.data_ptr(), self.B.data_ptr(), self.bias.data_ptr()
        g.C = g.residual = c_view.data_ptr()
        g.C_split, g.overflow_flag = s_view.data_ptr(), ovf.data_ptr()
        g.M, g.N, g.K, g.ldc, g.ldr = M, N, K, ldc, ldc
        snap = [t.clone() for t in (a_whole, c_whole, s_whole)]
        old = lib.t2h_gemm_split_force_config(cfg)
        try:
            assert lib.t2h_gemm_split_tile_config(ctypes.byref(g)) == cfg
            rc = lib.t2h_gemm_split_f32(ctypes.byref(g), None)
        finally:
            lib.t2h_gemm_split_force_config(old)
        assert rc == 0, lib.emu_last_error()
        band = G.band_of(c_whole, M)
        G.assert_bands_untouched(c_whole, band, M, snap[1], self.C0, N, what='C')                       # P2
        G.assert_bands_untouched(s_whole, G.band_of(s_whole, M), M, snap[2], what='C_split')            # P2
        assert torch.equal(a_whole, snap[0]), 'the A operand was written'
        return G.bits(c_view).clone(), s_view.clone(), int(ovf[0])

    def check_accuracy(self, c_bits, s_rows):                                                           # P1
        got = c_bits.view(torch.float32)
        err = (got.double() - self.ref).abs()
        if self.x8:
            assert (err <= 2e-6 * self.scale + 1e-6).all(), (err / self.scale).max().item()
        else:
            # (the bound's |ref| is a @ w.T + b WITHOUT the residual, as in test_gpu_split.test_gemm_split)
            assert (err <= 2e-5 + 2e-5 * self.lin.abs()).all(), err.max().item()
        if self.x8_out:
            hi, h8, l8 = ops.unpack_x8_rows_host(s_rows, self.M, self.N, self.so)
            whi, wh8, wl8 = x8_planes_host(got, self.so)
            assert torch.equal(hi, whi) and torch.equal(h8, wh8) and torch.equal(l8, wl8)
        else:
            assert torch.equal(s_rows, ops.pack_split_rows_host(got).view_as(s_rows))

    def spiked_residual(self, value):
        r = self.res.clone()
        r[self.M - 1, self.N - 1] = value
        return r


@pytest.mark.parametrize('x8', [False, True], ids=['fp16-planes', 'x8'])
@pytest.mark.parametrize('cfg', [0, 2, 6, 9])
@pytest.mark.parametrize('M', [17, 65, 129])
def test_emulated_gemm_partial_row_tiles_inside_longer_buffers(lib, M, cfg, x8):
    case = GemmCase(M, 64, 64, x8, x8_out=x8 and cfg == 9)
    c0, s0, ovf0 = case.launch(lib, cfg, poison=False)
    case.check_accuracy(c0, s0)                                                                         # P1 (P2 inside)
    c1, s1, ovf1 = case.launch(lib, cfg, poison=True)
    assert ovf0 == 0 and ovf1 == 0, (ovf0, ovf1)                                                        # P3
    assert torch.equal(c0, c1) and torch.equal(s0, s1), 'the result depends on what lies beyond the extent'
    # P4: one flagged value at (M - 1, N - 1), through the residual
    assert case.launch(lib, cfg, True, case.spiked_residual(1.0e5))[2] & 1
    if case.x8_out:
        v = 1.5 * 448.0 / case.so + 2.0 * float(case.ref.abs().max()) + 5.0
        assert v < 65504.0 and case.launch(lib, cfg, True, case.spiked_residual(v))[2] == 2


# ---- the row producers


def _producer(fn, rows, C, x, out_poison, poison):
    """out rows [rows, C/32, 2, 32] of fn(x_view_ptr, out_ptr, ovf_ptr) with x and out between bands -> (out, overflow)"""
    x_whole, x_view = G.banded(rows, (C, ), torch.float32, 'cpu', 16, f32_poison if poison else 0)
    x_view.copy_(x)
    o_whole, o_view = G.banded(rows, (C // 32, 2, 32), torch.int16, 'cpu', 16, out_poison if poison else 0)
    o_view.zero_()
    ovf = torch.zeros(1, dtype=torch.int32)
    snap_x, snap_o = x_whole.clone(), o_whole.clone()
    fn(x_view.data_ptr(), o_view.data_ptr(), ovf.data_ptr())
    G.assert_bands_untouched(o_whole, G.band_of(o_whole, rows), rows, snap_o, what='producer output')   # P2
    assert torch.equal(G.bits(x_whole), G.bits(snap_x))
    return o_view.clone(), int(ovf[0])


def _both_fills(fn, rows, C, x, out_poison):
    o0, f0 = _producer(fn, rows, C, x, out_poison, False)
    o1, f1 = _producer(fn, rows, C, x, out_poison, True)
    assert f0 == 0 and f1 == 0 and torch.equal(o0, o1)                                                  # P3
    return o0


@pytest.mark.parametrize('rows', [1, 37])
def test_emulated_split_row_producers_inside_longer_buffers(lib, rows):
    C = 512
    x = rnd(rows, C, seed=41) * 1.2
    s = ops.x8_scale_for(float(x.abs().max()))
    assert float(x.abs().max()) * s < 448.0

    def split(xp, op, fp):
        assert lib.t2h_split_rows_f32(xp, C, op, rows, C, fp, None) == 0, lib.emu_last_error()

    def split_x8(xp, op, fp):
        assert lib.t2h_split_rows_x8_f32(xp, C, op, rows, C, s, fp, None) == 0, lib.emu_last_error()

    got = _both_fills(split, rows, C, x, G.SPLIT_INF)
    assert torch.equal(got, ops.pack_split_rows_host(x).view_as(got))                                   # P1
    got = _both_fills(split_x8, rows, C, x, G.x8_poison())
    assert torch.equal(got.view(torch.uint8), x8_rows_host(x, s).view(torch.uint8))                      # P1
    x4 = x.clone()                                                                                      # P4
    x4[rows - 1, C - 1] = 1.0e5
    assert _producer(split, rows, C, x4, G.SPLIT_INF, True)[1] == 1
    assert _producer(split_x8, rows, C, x4, G.x8_poison(), True)[1] == 1
    x4[rows - 1, C - 1] = 1.5 * 448.0 / s
    assert _producer(split_x8, rows, C, x4, G.x8_poison(), True)[1] == 2


@pytest.mark.parametrize('rows', [1, 37])
def test_emulated_layernorm_producers_inside_longer_buffers(rows):
    norm = build_emu.load('norm.hip')
    C = 512
    x = rnd(rows, C, seed=42) * 2.0 + 0.3
    g, b = rnd(C, seed=43) * 0.2 + 1.0, rnd(C, seed=44) * 0.1
    # (the bit-exact reference is the fp32 LayerNorm kernel of the same file, itself within 1e-5 of fp64, as in
    # test_split_producers_are_bitwise_the_split_of_the_fp32_result: the property is 'the planes OF the fp32 result')
    y = torch.zeros(rows, C)
    assert norm.t2h_layernorm_f32(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), rows, C, 1e-5, None) == 0
    assert (y - F.layer_norm(x.double(), (C, ), g.double(), b.double(), 1e-5)).abs().max().item() < 1e-5
    s = ops.x8_scale_for(float(y.abs().max()))
    assert float(y.abs().max()) * s < 448.0

    def ln_split(gamma):
        def fn(xp, op, fp):
            rc = norm.t2h_layernorm_split_f32(xp, gamma.data_ptr(), b.data_ptr(), op, rows, C, 1e-5, fp, None)
            assert rc == 0, norm.emu_last_error()
        return fn

    def ln_x8(gamma):
        def fn(xp, op, fp):
            rc = norm.t2h_layernorm_x8_f32(xp, gamma.data_ptr(), b.data_ptr(), op, rows, C, 1e-5, s, fp, None)
            assert rc == 0, norm.emu_last_error()
        return fn

    got = _both_fills(ln_split(g), rows, C, x, G.SPLIT_INF)
    assert torch.equal(got, ops.pack_split_rows_host(y).view_as(got))                                   # P1
    got = _both_fills(ln_x8(g), rows, C, x, G.x8_poison())
    assert torch.equal(got.view(torch.uint8), x8_rows_host(y, s).view(torch.uint8))                      # P1
    # P4: every row's last column sits at the mean of its row (it normalises to ~0) but for the spike at
    # x[rows - 1, C - 1], which normalises to ~sqrt(C - 1) = 22.6; the last column's gain lifts that ONE value out of
    # range -- and no other, asserted on the reference -- so the word holds exactly its bit
    x4 = x.clone()
    x4[:, C - 1] = x4[:, :C - 1].mean(dim=1)
    x4[rows - 1, C - 1] = 1.0e4
    for limit, make, poison, bit in ((65504.0, ln_split, G.SPLIT_INF, 1), (65504.0, ln_x8, G.x8_poison(), 1),
                                     (448.0 / s, ln_x8, G.x8_poison(), 2)):
        g4 = g.clone()
        g4[C - 1] = 1.6 * limit / (C - 1) ** 0.5
        ref = F.layer_norm(x4, (C, ), g4, b, 1e-5).abs()
        assert float(ref[rows - 1, C - 1]) >= 1.2 * limit
        ref[rows - 1, C - 1] = 0.0
        assert float(ref.max()) < 0.8 * (min(limit, 448.0 / s) if make is ln_x8 else limit)
        assert _producer(make(g4), rows, C, x4, poison, True)[1] == bit


@pytest.mark.parametrize('rows', [1, 37])
def test_emulated_gather_rows_inside_longer_buffers(rows):
    """t2h_gather_rows (finish_tail's compaction) of fp32 rows and of split rows: the source, the index list and the
    output between bands; list entries behind n_rows and in the bands name a VALID row (they must not be read, and a
    test must not make an out-of-range read out of it if they are)."""
    misc = build_emu.load('misc.hip')
    n_src, C = 96, 512
    idx = torch.randperm(n_src, generator=torch.Generator().manual_seed(45))[:rows].to(torch.int32)
    for src in (rnd(n_src, C, seed=46), ops.pack_split_rows_host(rnd(n_src, C, seed=47))):
        tail, row_bytes = tuple(src.shape[1:]), src[0].numel() * src.element_size()
        fp32 = src.dtype == torch.float32
        outs = []
        for poison in (False, True):
            s_whole, s_view = G.banded(n_src, tail, src.dtype, 'cpu', 16, (f32_poison if fp32 else G.SPLIT_INF) if poison else 0)
            s_view.copy_(src)
            i_whole, i_view = G.banded(rows + 8, (), torch.int32, 'cpu', 16, VALID_ROW if poison else 0)
            i_view[:rows] = idx
            o_whole, o_view = G.banded(rows, tail, src.dtype, 'cpu', 16, (f32_poison if fp32 else G.SPLIT_INF) if poison else 0)
            o_view.zero_()
            snap = [t.clone() for t in (s_whole, i_whole, o_whole)]
            rc = misc.t2h_gather_rows(s_view.data_ptr(), i_view.data_ptr(), o_view.data_ptr(), rows, row_bytes, None)
            assert rc == 0, misc.emu_last_error()
            G.assert_bands_untouched(o_whole, G.band_of(o_whole, rows), rows, snap[2], what='gathered rows')       # P2
            assert torch.equal(G.bits(s_whole), G.bits(snap[0])) and torch.equal(i_whole, snap[1])
            outs.append(G.bits(o_view).clone())
        assert torch.equal(outs[0], G.bits(src[idx.long()]))                                            # P1
        assert torch.equal(outs[0], outs[1])                                                            # P3 (no range guard here: no P4)
