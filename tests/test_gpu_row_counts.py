"""The sampler's GEMM chain at the row counts its rounds really run (-m gpu), every buffer inside a LONGER one.

engine.SamplerNet.finish_tail evaluates proj / LN2 / fc1 / fc2 on m = 1..256 compacted rows of buffers that hold 256
(the rows behind m are stale leftovers of earlier rounds); with finished samples leaving the batch every layer runs
on M = 512 k rows of the full-batch buffers, the later samples' rows and value planes right behind.  For every case
(tests/guard_util.py):

  P1  accuracy against a reference of the same operation, with the bounds of test_gpu_split.py / test_gpu_x8.py;
  P2  every output sits between guard bands that are byte-identical after the launch;
  P3  every input the product keeps in a longer buffer sits between bands too: zero bands and poisoned bands give
      bitwise-equal outputs and leave the sticky overflow word 0;
  P4  where the launch has a range guard (a split-row / x8 / Vt output): ONE out-of-range value inside the extent, at
      row M - 1 and the last column, raises its bit -- P3's zero is not vacuous.  (proj / fc2 write fp32 rows only:
      no guard runs, nothing to flag.)

The CPU twin (exact bands in host memory, the kernels' source through tests/emu) is test_row_counts_emulated.py."""
import ctypes
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import guard_util as G
from split_ref import emulate_x8 as _emulate, pack_vt_host as _pack_vt_host, x8_planes_host as _x8_planes_host
from text2human_amd import _lib, engine, ops, synthetic, weights

pytestmark = pytest.mark.gpu
DEV = 'cuda'
VALID_ROW = 3   # what the index list holds behind n_rows and in its bands: a row that exists
BAND = 256   # rows: the tallest tile (256 x 128) fits into a band, so a store of unmasked tile rows lands in it


def _rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def f32_poison(whole):
    """rows alternate between the NaN pattern (invisible to a `>=` range guard, fatal in a sum) and 1e30 (visible)"""
    G.fill_bits(whole, G.F32_NAN)
    G.bits(whole)[1::2] = G.F32_BIG


def rows_poison(x8):
    return G.x8_poison() if x8 else G.SPLIT_INF


@functools.lru_cache(maxsize=None)
def _problem(m_max, N, K, x8, seed):
    """operands and the reference of one Linear at m_max rows, shared by every row count (rows are independent: the
    case at M rows is the first M rows); activations randn * 1.2, weights at scale 0.06, x8 scales from their maxima"""
    p = types.SimpleNamespace(N=N, K=K, x8=x8)
    p.a, p.w, p.b, p.r = _rnd(m_max, K, seed=seed) * 1.2, _rnd(N, K, seed=seed + 1, scale=0.06), _rnd(N, seed=seed + 2), _rnd(m_max, N, seed=seed + 3)
    p.scale = p.a.double().abs() @ p.w.double().abs().t()
    if x8:
        p.sa, p.sw = ops.x8_scale_for(float(p.a.abs().max())), ops.x8_scale_for(float(p.w.abs().max()), 256.0)
        assert float(p.a.abs().max()) * p.sa < 448.0 and float(p.w.abs().max()) * p.sw < 448.0
        p.lin = _emulate(p.a, p.w, p.sa, p.sw) + p.b.double()
        p.a_rows, p.w_rows = ops.split_rows_x8(p.a.to(DEV), p.sa), ops.split_rows_x8(p.w.to(DEV), p.sw)
    else:
        p.lin = p.a.double() @ p.w.double().t() + p.b.double()
        p.a_rows, p.w_rows = ops.split_rows(p.a.to(DEV)), ops.pack_split_rows_host(p.w).to(DEV)
    p.b_dev = p.b.to(DEV)
    assert ops.split_overflow_bits(reset=True) == 0
    return p


def _a_rows(p, a):
    """device rows of an activation matrix in p's operand format (P4: the producer's own flag is cleared)"""
    rows = ops.split_rows_x8(a.to(DEV), p.sa) if p.x8 else ops.split_rows(a.to(DEV))
    ops.split_overflow_bits(reset=True)
    return rows


def _tile_config(p, M, vt=False):
    g = _lib.GemmSplitArgs()
    g.M, g.N, g.K, g.fmt, g.bias = M, p.N, p.K, int(p.x8), p.b_dev.data_ptr()
    if vt:
        g.Vt, g.vt_col0, g.vt_T, g.vt_hd = p.w_rows.data_ptr(), p.N - 512, 512, 64   # (any non-NULL pointer: not launched)
    return _lib.load().t2h_gemm_split_tile_config(ctypes.byref(g))


def _launch(p, M, poison, *, act=ops.ACT_NONE, residual=None, want_c=True, want_split=False, out_x8_scale=None,
            vt_images=0, ld_extra=0, a_rows=None, bias=None):
    """One t2h_gemm_split_f32 launch on M rows with every buffer between bands (zero, or poisoned) -> namespace of the
    outputs' bits and the overflow word.  residual [M, N] (CPU): added IN PLACE (C = residual = the same rows).
    P2 -- the bands of every output, the whole A buffer -- is asserted here."""
    N, K = p.N, p.K
    r = types.SimpleNamespace(c=None, s=None, vt=None)
    a_whole, a_view = G.banded(M, (K // 32, 2, 32), torch.int16, DEV, BAND, rows_poison(p.x8) if poison else 0)
    a_view.copy_(p.a_rows[:M] if a_rows is None else a_rows)
    held, c_view, s_view, vt_view = [('A', a_whole, a_view, None)], None, None, None
    if want_c:
        c0 = 8 if ld_extra else 0
        c_whole, c_rows = G.banded(M, (N + ld_extra, ), torch.float32, DEV, BAND, f32_poison if poison else 0)
        if poison:
            f32_poison(c_rows)                       # (the columns beside the extent too)
        c_view = c_rows[:, c0:c0 + N]
        c_view.copy_(residual) if residual is not None else c_view.zero_()
        held.append(('C', c_whole, c_view, (c0, N)))
    if want_split:
        s_whole, s_view = G.banded(M, (N // 32, 2, 32), torch.int16, DEV, BAND,
                                   rows_poison(out_x8_scale is not None) if poison else 0)
        s_view.zero_()
        held.append(('C_split', s_whole, s_view, None))
    if vt_images:
        vt_whole, vt_view = G.banded(vt_images, (8, 2, 64, 512), torch.int16, DEV, 1, G.SPLIT_INF if poison else 0)
        vt_view.zero_()
        held.append(('Vt', vt_whole, vt_view, None))
    snaps = [whole.clone() for _, whole, _, _ in held]
    ops.split_overflow_bits(reset=True)
    ops.gemm_split(a_view, p.w_rows, M, N, K, out=c_view, out_split=s_view, bias=p.b_dev if bias is None else bias,
                   residual=c_view if residual is not None else None, act=act, vt=vt_view,
                   vt_col0=N - 512 if vt_images else 0, vt_T=512 if vt_images else 0,
                   x8=(p.sa, p.sw) if p.x8 else None, out_x8_scale=out_x8_scale)
    r.ovf = ops.split_overflow_bits(reset=True)
    for (what, whole, view, cols), snap in zip(held, snaps):
        if what == 'A':
            assert torch.equal(whole, snap), 'the A operand was written'
        else:
            rows = view.shape[0]
            G.assert_bands_untouched(whole, G.band_of(whole, rows), rows, snap, *(cols or ()), what=what)
    r.c = G.bits(c_view).clone() if want_c else None
    r.s = s_view.clone() if want_split else None
    r.vt = vt_view.clone() if vt_images else None
    return r


def _same_bits(r0, r1):
    for name in ('c', 's', 'vt'):
        u, v = getattr(r0, name), getattr(r1, name)
        assert (u is None and v is None) or torch.equal(u, v), f'{name}: the result depends on what lies beyond the extent'
    assert r0.ovf == 0 and r1.ovf == 0, (r0.ovf, r1.ovf)


def _check_linear(p, M, c_bits, add=None, act=ops.ACT_NONE):
    """P1 of an fp32 output: the bounds of test_gpu_split.test_gemm_split / test_gpu_x8 for this operand format"""
    got, lin = c_bits.view(torch.float32).cpu().double(), p.lin[:M]
    ref = F.gelu(lin) if act == ops.ACT_GELU else lin
    err = (got - (ref + add.double() if add is not None else ref)).abs()
    print(f'N={p.N} K={p.K} M={M} x8={p.x8}: max err {err.max().item():.3g}')
    if not p.x8:   # (the bound's |ref| is a @ w.T + b without the residual, as in test_gpu_split.test_gemm_split)
        assert (err <= 2e-5 + 2e-5 * lin.abs()).all(), err.max().item()
    elif act == ops.ACT_GELU:
        assert err.max().item() < 1e-5                       # (test_gemm_x8_few_rows_kernel_and_epilogues' bound for it)
    else:
        assert (err <= 2e-6 * p.scale[:M] + 1e-6).all(), (err / p.scale[:M]).max().item()


def _check_planes(c_bits, s_rows, out_x8_scale):
    """the split-row output carries the planes of the fp32 output of the same launch, bit for bit"""
    got = c_bits.view(torch.float32).cpu()
    M, N = got.shape
    if out_x8_scale is None:
        assert torch.equal(s_rows.cpu(), ops.pack_split_rows_host(got).view_as(s_rows.cpu()))
    else:
        hi, h8, l8 = ops.unpack_x8_rows_host(s_rows, M, N, out_x8_scale)
        whi, wh8, wl8 = _x8_planes_host(got, out_x8_scale)
        assert torch.equal(hi, whi) and torch.equal(h8, wh8) and torch.equal(l8, wl8)


def _spiked_row(p, M, target):
    """activations whose row M - 1 is c * sign(w[N - 1]): output (M - 1, N - 1) becomes ~target; asserted here: no other
    output of that row reaches 0.8 * target (all other rows are unchanged)"""
    a = p.a[:M].clone()
    wl = p.w[p.N - 1]
    a[M - 1] = torch.sign(wl) * (target / float(wl.abs().sum()))
    out = a[M - 1].double() @ p.w.double().t() + p.b.double()
    assert float(out[p.N - 1]) >= 0.95 * target and float(out[:p.N - 1].abs().max()) < 0.8 * target
    return a


# ---- (a) the tail's row counts on the automatic dispatch

TAIL_M = [1, 15, 16, 17, 63, 64, 65, 100, 128, 129, 200, 255, 256]


@pytest.mark.parametrize('x8', [False, True], ids=['fp16-planes', 'x8'])
@pytest.mark.parametrize('M', TAIL_M)
def test_tail_linears_at_every_kind_of_row_count(M, x8):
    """finish_tail's three Linears at m compacted rows: the few-rows kernel (configuration 9, 16-row tiles) up to 64
    rows, the 128 x 64 tile with the in-block K split (6) and a partial last row tile from 65 to 256."""
    want_cfg = 9 if M <= 64 else 6
    # proj: N = 512, K = 512, residual in place
    p = _problem(256, 512, 512, x8, 100)
    assert _tile_config(p, M) == want_cfg
    r0, r1 = (_launch(p, M, poison, residual=p.r[:M]) for poison in (False, True))
    _check_linear(p, M, r0.c, add=p.r[:M])
    _same_bits(r0, r1)
    # fc2: N = 512, K = 2048, residual in place
    p = _problem(256, 512, 2048, x8, 110)
    assert _tile_config(p, M) == want_cfg
    r0, r1 = (_launch(p, M, poison, residual=p.r[:M]) for poison in (False, True))
    _check_linear(p, M, r0.c, add=p.r[:M])
    _same_bits(r0, r1)
    # fc1: N = 2048, K = 512, GELU, fp32 rows + split rows (x8 operands: x8 rows) out
    p = _problem(256, 2048, 512, x8, 120)
    assert _tile_config(p, M) == want_cfg
    so = ops.x8_scale_for(float(F.gelu(p.lin).abs().max())) if x8 else None
    assert not x8 or float(F.gelu(p.lin).abs().max()) * so < 448.0
    kw = dict(act=ops.ACT_GELU, want_split=True, out_x8_scale=so)
    r0, r1 = (_launch(p, M, poison, **kw) for poison in (False, True))
    _check_linear(p, M, r0.c, act=ops.ACT_GELU)
    _check_planes(r0.c, r0.s, so)
    _same_bits(r0, r1)
    # P4
    if not x8:
        assert _launch(p, M, True, a_rows=_a_rows(p, _spiked_row(p, M, 1.0e5)), **kw).ovf == 1
    else:
        bias = p.b.clone()
        bias[p.N - 1] = 1.0e5                                 # (x8 activations cannot carry a product to 65504)
        assert _launch(p, M, True, bias=bias.to(DEV), **kw).ovf & 1
        assert _launch(p, M, True, a_rows=_a_rows(p, _spiked_row(p, M, 1.5 * 448.0 / so)), **kw).ovf == 2


# ---- (b) forced tile configurations with partial tiles, x8 operands

_KS = {6: 2}   # K tiles a configuration consumes per step: launch_split requires K % (32 * KS) == 0


@pytest.mark.parametrize('cfg', [0, 2, 6, 8, 10])
@pytest.mark.parametrize('M,N,K', [(130, 192, 64), (321, 384, 256)])
def test_x8_tile_configurations_on_partial_tiles(M, N, K, cfg):
    """every tile configuration built for x8 operands with a partial last row tile (and, 256 x 128 / 128 x 64 tiles at
    N = 192 / 384, a partial column tile): fp32 rows with the residual in place at a leading dimension of N + 16, and
    the x8 rows of the same launch"""
    if K % (32 * _KS.get(cfg, 1)):
        pytest.skip(f'configuration {cfg} needs K % {32 * _KS.get(cfg, 1)} == 0')
    p = _problem(M, N, K, True, 200 + M)
    ref = p.lin + p.r.double()
    so = ops.x8_scale_for(float(ref.abs().max()))
    assert float(ref.abs().max()) * so < 448.0
    kw = dict(want_split=True, out_x8_scale=so, ld_extra=16)
    lib = _lib.load()
    lib.t2h_gemm_split_force_config(cfg)
    try:
        assert _tile_config(p, M) == cfg
        r0, r1 = (_launch(p, M, poison, residual=p.r, **kw) for poison in (False, True))
        res = p.r.clone()
        res[M - 1, N - 1] = 1.0e5
        f0 = _launch(p, M, True, residual=res, **kw).ovf
        res[M - 1, N - 1] = 1.5 * 448.0 / so + 2.0 * float(ref.abs().max()) + 5.0
        f1 = _launch(p, M, True, residual=res, **kw).ovf
    finally:
        lib.t2h_gemm_split_force_config(-1)
    _check_linear(p, M, r0.c, add=p.r)
    _check_planes(r0.c, r0.s, so)
    _same_bits(r0, r1)
    assert f0 & 1 and f1 == 2, (f0, f1)                                                                  # P4


# ---- (c) a batch that has shrunk to k of its samples


@pytest.mark.parametrize('x8', [False, True], ids=['fp16-planes', 'x8'])
@pytest.mark.parametrize('k', [3, 5, 7])
def test_layer_linears_on_a_prefix_of_the_batch(k, x8):
    """hidden(active=k): M = 512 k rows of the full-batch buffers -- q|k|v with the value columns routed to the
    transposed planes (one more image's planes on either side) and fc2 with the residual in place"""
    M, C, T, H = 512 * k, 512, 512, 8
    p = _problem(3584, 3 * C, C, x8, 300)
    assert _tile_config(p, M, vt=True) == 0                  # 128 x 64 tiles (M = 512 k is no multiple of 256 x ...)
    full = _launch(p, M, False)                              # fp32 rows of the same arithmetic
    _check_linear(p, M, full.c)
    kw = dict(want_c=False, want_split=True, vt_images=k)
    r0, r1 = (_launch(p, M, poison, **kw) for poison in (False, True))
    _same_bits(r0, r1)
    f32 = full.c.view(torch.float32).cpu()
    want, got = ops.pack_split_rows_host(f32), r0.s.cpu()
    assert torch.equal(got[:, :2 * C // 32], want[:, :2 * C // 32])
    assert (got[:, 2 * C // 32:] == 0).all(), 'value columns must not be written as split rows'
    assert torch.equal(r0.vt.cpu(), _pack_vt_host(f32[:, 2 * C:].contiguous(), k, T, H))
    if not x8:                                                                                           # P4 (the Vt store's guard)
        assert _launch(p, M, True, a_rows=_a_rows(p, _spiked_row(p, M, 1.0e5)), **kw).ovf == 1
    else:
        bias = p.b.clone()
        bias[p.N - 1] = 1.0e5
        assert _launch(p, M, True, bias=bias.to(DEV), **kw).ovf == 1
    # fc2
    p = _problem(3584, C, 4 * C, x8, 310)
    assert _tile_config(p, M) == 6
    r0, r1 = (_launch(p, M, poison, residual=p.r[:M]) for poison in (False, True))
    _check_linear(p, M, r0.c, add=p.r[:M])
    _same_bits(r0, r1)


# ---- (d) the row producers


def _producer(fn, rows, C, x, out_poison, poison):
    """split rows [rows, C/32, 2, 32] of fn(x view, out view), both between bands -> (out, overflow word)"""
    x_whole, x_view = G.banded(rows, (C, ), torch.float32, DEV, 16, f32_poison if poison else 0)
    x_view.copy_(x)
    o_whole, o_view = G.banded(rows, (C // 32, 2, 32), torch.int16, DEV, 16, out_poison if poison else 0)
    o_view.zero_()
    snap_x, snap_o = x_whole.clone(), o_whole.clone()
    ops.split_overflow_bits(reset=True)
    fn(x_view, o_view)
    flag = ops.split_overflow_bits(reset=True)
    G.assert_bands_untouched(o_whole, G.band_of(o_whole, rows), rows, snap_o, what='producer output')   # P2
    assert torch.equal(G.bits(x_whole), G.bits(snap_x))
    return o_view.clone(), flag


def _both_fills(fn, rows, C, x, out_poison):
    o0, f0 = _producer(fn, rows, C, x, out_poison, False)
    o1, f1 = _producer(fn, rows, C, x, out_poison, True)
    assert f0 == 0 and f1 == 0 and torch.equal(o0, o1)                                                  # P3
    return o0


def _x8_bytes(x, s):
    """x8 rows of x on the host, as (hi, hi8, lo8) numbers (test_gpu_x8._x8_planes_host)"""
    return _x8_planes_host(x, s)


@pytest.mark.parametrize('C', [512, 2048])
@pytest.mark.parametrize('rows', [1, 37, 65, 255])
def test_split_row_producers_inside_longer_buffers(rows, C):
    x = _rnd(rows, C, seed=400 + rows) * 1.2
    s = ops.x8_scale_for(float(x.abs().max()))
    assert float(x.abs().max()) * s < 448.0
    split = lambda xv, ov: ops.split_rows(xv, out=ov)            # noqa: E731
    split_x8 = lambda xv, ov: ops.split_rows_x8(xv, s, out=ov)   # noqa: E731
    got = _both_fills(split, rows, C, x.to(DEV), G.SPLIT_INF)
    assert torch.equal(got.cpu(), ops.pack_split_rows_host(x).view_as(got.cpu()))                       # P1
    got = _both_fills(split_x8, rows, C, x.to(DEV), G.x8_poison())
    assert all(torch.equal(u, v) for u, v in zip(ops.unpack_x8_rows_host(got, rows, C, s), _x8_bytes(x, s)))
    x4 = x.clone()                                                                                      # P4
    x4[rows - 1, C - 1] = 1.0e5
    assert _producer(split, rows, C, x4.to(DEV), G.SPLIT_INF, True)[1] == 1
    assert _producer(split_x8, rows, C, x4.to(DEV), G.x8_poison(), True)[1] == 1
    x4[rows - 1, C - 1] = 1.5 * 448.0 / s
    assert _producer(split_x8, rows, C, x4.to(DEV), G.x8_poison(), True)[1] == 2


@pytest.mark.parametrize('rows', [1, 37, 65, 255])
def test_layernorm_producers_inside_longer_buffers(rows):
    C = 512
    x = _rnd(rows, C, seed=420 + rows) * 2.0 + 0.3
    g, b = _rnd(C, seed=421) * 0.2 + 1.0, _rnd(C, seed=422) * 0.1
    gd, bd = g.to(DEV), b.to(DEV)
    y = ops.layernorm(x.to(DEV), gd, bd).cpu()
    assert (y - F.layer_norm(x.double(), (C, ), g.double(), b.double(), 1e-5)).abs().max().item() < 1e-5
    s = ops.x8_scale_for(float(y.abs().max()))
    assert float(y.abs().max()) * s < 448.0
    ln_split = lambda gamma: lambda xv, ov: ops.layernorm_split(xv, gamma, bd, ov)     # noqa: E731
    ln_x8 = lambda gamma: lambda xv, ov: ops.layernorm_x8(xv, gamma, bd, ov, s)        # noqa: E731
    got = _both_fills(ln_split(gd), rows, C, x.to(DEV), G.SPLIT_INF)
    assert torch.equal(got.cpu(), ops.pack_split_rows_host(y).view_as(got.cpu()))                       # P1
    got = _both_fills(ln_x8(gd), rows, C, x.to(DEV), G.x8_poison())
    assert all(torch.equal(u, v) for u, v in zip(ops.unpack_x8_rows_host(got, rows, C, s), _x8_bytes(y, s)))
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
        assert _producer(make(g4.to(DEV)), rows, C, x4.to(DEV), poison, True)[1] == bit


@pytest.mark.parametrize('rows', [1, 37, 65, 255])
def test_gather_rows_inside_longer_buffers(rows):
    """t2h_gather_rows (finish_tail's compaction) of fp32 rows and of split rows: source, index list and output
    between bands; list entries behind n_rows and in the bands name a VALID row, never an out-of-range one"""
    n_src, C = 1024, 512
    idx = torch.randperm(n_src, generator=torch.Generator().manual_seed(430 + rows))[:rows].to(torch.int32)
    for src in (_rnd(n_src, C, seed=431), ops.pack_split_rows_host(_rnd(n_src, C, seed=432))):
        tail, fp32 = tuple(src.shape[1:]), src.dtype == torch.float32
        fill = f32_poison if fp32 else G.SPLIT_INF
        outs = []
        for poison in (False, True):
            s_whole, s_view = G.banded(n_src, tail, src.dtype, DEV, 16, fill if poison else 0)
            s_view.copy_(src)
            i_whole, i_view = G.banded(rows + 8, (), torch.int32, DEV, 16, VALID_ROW if poison else 0)
            i_view[:rows] = idx.to(DEV)
            o_whole, o_view = G.banded(rows, tail, src.dtype, DEV, 16, fill if poison else 0)
            o_view.zero_()
            snap = [t.clone() for t in (s_whole, i_whole, o_whole)]
            ops.gather_rows(s_view, i_view, rows, out=o_view)
            torch.cuda.synchronize()
            G.assert_bands_untouched(o_whole, G.band_of(o_whole, rows), rows, snap[2], what='gathered rows')       # P2
            assert torch.equal(G.bits(s_whole), G.bits(snap[0])) and torch.equal(i_whole, snap[1])
            outs.append(G.bits(o_view).clone())
        assert torch.equal(outs[0].cpu(), G.bits(src[idx.long()]))                                      # P1
        assert torch.equal(outs[0], outs[1])                                                            # P3 (no range guard here: no P4)


# ---- (e) attention on a prefix of the batch


@functools.lru_cache(maxsize=None)
def _attention_inputs():
    B, T, H, C = 5, 512, 8, 512
    qkv = _rnd(B * T, 3 * C, seed=500) * 1.3
    q, k, v = [t.view(B, T, H, 64).transpose(1, 2).double() for t in qkv.split(C, dim=1)]
    ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(1, 2).reshape(B * T, C)
    y32 = ops.mha_noncausal(qkv.to(DEV), B, T, H).cpu().double()
    return ops.split_rows(qkv.to(DEV)), _pack_vt_host(qkv[:, 2 * C:].contiguous(), B, T, H).to(DEV), ref, y32


@pytest.mark.parametrize('form', [1, 2])
def test_attention_on_the_first_images_of_a_larger_batch(form):
    """mha_split (fp32 rows, split rows) and mha_split_x8 on images 0..2 of 5-image q|k / Vt / y buffers, both forms of
    the kernel: images 3, 4 poisoned on the input side, their output rows bands -- bit for bit the first 3 images of a
    clean 5-image run of the same form"""
    B, k, T, H, C, s8 = 5, 3, 512, 8, 512, 64.0
    M = k * T
    qk5, vt5, ref, y32 = _attention_inputs()
    lib = _lib.load()
    kinds = ('fp32', 'split', 'x8')

    def run(kind, qk, vt, n_img, out):
        ops.split_overflow_bits(reset=True)
        if kind == 'fp32':
            ops.mha_split(qk, 3 * C, vt, n_img, T, H, out=out)
        elif kind == 'split':
            ops.mha_split(qk, 3 * C, vt, n_img, T, H, out_split=out)
        else:
            ops.mha_split_x8(qk, 3 * C, vt, n_img, T, H, out, s8)
        return ops.split_overflow_bits(reset=True)

    def empty(kind):
        return torch.zeros(B * T, C, device=DEV) if kind == 'fp32' else ops.split_rows_empty(B * T, C, DEV).zero_()

    lib.t2h_mha_split_force_form(form)
    try:
        clean = {}
        for kind in kinds:
            clean[kind] = empty(kind)
            assert run(kind, qk5, vt5, B, clean[kind]) == 0
        # P1 (test_mha_split_matches_fp64_reference...'s bound; the other outputs are planes of these numbers)
        e32, es = (y32 - ref).abs().max().item(), (clean['fp32'].cpu().double() - ref).abs().max().item()
        assert es < 5e-6 + 2 * e32, (es, e32)
        assert torch.equal(clean['split'], ops.split_rows(clean['fp32']))
        hi = ops.unpack_x8_rows_host(clean['x8'], B * T, C, s8)[0]
        assert torch.equal(hi, clean['fp32'].cpu().half().float()) and float(hi.abs().max()) * s8 < 448.0
        ops.split_overflow_bits(reset=True)
        for poison in (False, True):
            qk, vt = qk5.clone(), vt5.clone()
            G.fill_bits(qk[M:], G.SPLIT_INF if poison else 0)
            G.fill_bits(vt[k:], G.SPLIT_INF if poison else 0)
            for kind in kinds:
                out = empty(kind)
                if poison:
                    f32_poison(out[M:]) if kind == 'fp32' else G.fill_bits(out[M:], rows_poison(kind == 'x8'))
                snap = out.clone()
                assert run(kind, qk, vt, k, out) == 0                                                   # P3
                G.assert_bands_untouched(out, 0, M, snap, what=f'attention output ({kind})')            # P2
                assert torch.equal(G.bits(out[:M]), G.bits(clean[kind][:M])), kind                      # P3
        # P4: value column (head 7, dim 63) of image 2 = 65520 = fp16 max + 32768 / 2048 in the two planes -> every
        # query of the image, row M - 1 among them, gets ~65520 in the last column; x8: 14 -> 14 * 64 >= 448
        for kind, (hi_v, lo_v), want in (('split', (65504.0, 32768.0), 1), ('x8', (14.0, 0.0), 2)):
            vt = vt5.clone()
            vt[k - 1, H - 1, 0, 63] = torch.tensor(hi_v, dtype=torch.float16).view(torch.int16).item()
            vt[k - 1, H - 1, 1, 63] = torch.tensor(lo_v, dtype=torch.float16).view(torch.int16).item()
            assert run(kind, qk5, vt, k, empty(kind)) == want
    finally:
        lib.t2h_mha_split_force_form(0)


# ---- (f) the chain itself


@functools.lru_cache(maxsize=None)
def _tail_net(x8):
    sd = synthetic.fill(synthetic.transformer_schema(18432, 1024, 18, 512, 3, 512, 18), seed=12)
    P = weights.Params(DEV)
    desc = weights.pack_transformer(P, sd, 'tf')
    gen = torch.Generator().manual_seed(21)
    idx = torch.randint(0, 18433, (2, 512), generator=gen)
    seg = torch.randint(0, 1024, (2, 512), generator=gen)
    tex = torch.randint(0, 18, (2, 512), generator=gen)
    args = (idx.to(DEV), seg.to(DEV), tex.to(DEV))
    net = engine.SamplerNet(P, desc, 8, 'tf', split=True, x8=x8)
    full = net.hidden(*args).clone()
    assert (net._x8 is not None) == x8
    return net, args, full


@pytest.mark.parametrize('x8', [False, True], ids=['fp16-planes', 'x8'])
@pytest.mark.parametrize('n_rows', [64, 65, 200, 256, 257])
def test_finish_tail_at_the_kernel_thresholds_with_stale_rows_behind(n_rows, x8):
    """SamplerNet.finish_tail on n_rows compacted rows = those rows of the full evaluation, to the bounds of
    test_last_layer_tail_on_the_changed_rows_only... (2e-5) and test_sampler_net_x8_against_the_oracle... (5e-5): two
    tilings of one arithmetic.  64: the few-rows kernel; 65, 200, 256: 128 x 64 tiles with the in-block K split;
    257: too many, the tail runs on the whole batch (bit for bit the full evaluation).  The buffers xc / yc / hc / uc
    hold 256 rows: what lies behind n_rows -- zeros, or NaN / 1e30 / inf -- neither changes a bit of the result nor
    raises the overflow word, and is not written.
    Measured max |got - full[rows]|: NOT RECORDED YET -- the test prints it for every case before it asserts (run with
    -s); whoever first runs this file on an MI355X writes the figures here."""
    net, args, full = _tail_net(x8)
    rows = torch.randperm(1024, generator=torch.Generator().manual_seed(600 + n_rows))[:n_rows].to(torch.int32).to(DEV)
    buf = net._buffers(1024, 512, args[0].device)
    names = ('xc', 'yc', 'hc', 'uc')
    results = []
    for poison in (False, True):
        m = min(n_rows, net.TRIM_MAX_ROWS)
        for name in names:
            stale = buf[name][m:] if n_rows <= net.TRIM_MAX_ROWS else buf[name]
            if name == 'xc':
                f32_poison(stale) if poison else stale.zero_()
            else:
                G.fill_bits(stale, rows_poison(x8) if poison else 0)
        snap = {name: buf[name].clone() for name in names}
        net.hidden(*args, defer_tail=True)
        ops.split_overflow_bits(reset=True)
        got, compact = net.finish_tail(rows, n_rows)
        assert ops.split_overflow_bits(reset=True) == 0
        results.append(got.clone())
        for name in names:                       # (n_rows > 256: the compact buffers are not used at all)
            keep = slice(m, None) if compact else slice(None)
            assert torch.equal(G.bits(buf[name][keep]), G.bits(snap[name][keep])), f'{name}: rows behind n_rows written'
    if n_rows > net.TRIM_MAX_ROWS:
        assert not compact and torch.equal(results[0], full)
    else:
        assert compact and results[0].shape == (n_rows, 512)
        err = (results[0] - full[rows.long()]).abs().max().item()
        print(f'finish_tail n_rows={n_rows} x8={x8}: max |got - full[rows]| = {err:.3g}')
        assert err < (5e-5 if x8 else 2e-5), err
    assert torch.equal(G.bits(results[0]), G.bits(results[1])), 'the tail depends on the stale rows behind n_rows'
