"""Thin tensor -> pointer wrappers over the C ABI (include/t2h_hip.h).

PyTorch-ROCm is used for device memory, streams and nothing else: every
function here checks dtype / device / contiguity, takes raw device pointers and
the current HIP stream, and calls into libt2h_hip.so.
"""
import collections
import ctypes
import numbers
import os

import numpy as np
import torch

from . import _lib, options, schedule
from ._lib import GemmArgs, check

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
PRO_NONE, PRO_SWISH = 0, 1


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the sticky overflow word of the split-row producers (include/t2h_hip.h): owned HERE, one int32 in
# device memory per (device, stream) plus a pinned host word the asynchronous read-back lands in.  Models
# driven on different streams (or threads, each on its own stream) neither see nor clear each other's flag.
_ovf_slots = {}


def _ovf_slot():
    dev = torch.cuda.current_device()
    key = (dev, torch.cuda.current_stream().cuda_stream)
    slot = _ovf_slots.get(key)
    if slot is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.T2HError('the overflow flag of this stream must exist before a capture begins: call '
                                'ops.split_overflow(reset=True) on the stream first')
        slot = _ovf_slots[key] = (torch.zeros(1, dtype=torch.int32, device=f'cuda:{dev}'),
                                  torch.zeros(1, dtype=torch.int32).pin_memory())
    return slot


def overflow_flag():
    """Device pointer of the current stream's overflow word (allocated, zeroed, at first use)."""
    return ctypes.c_void_p(_ovf_slot()[0].data_ptr())


def release_overflow_flag(stream=None):
    """Forgets the overflow word of `stream` (default: the current one), e.g. before the stream is destroyed:
    a later stream that reuses the handle then starts from a fresh, zeroed word."""
    st = stream if stream is not None else torch.cuda.current_stream()
    _ovf_slots.pop((torch.cuda.current_device(), st.cuda_stream), None)


def _chk_f32(*ts):
    for t in ts:
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_cuda:
            raise TypeError(f'expected CUDA float32 tensor, got {t.dtype} on {t.device}')


def _chk_i64(*ts):
    for t in ts:
        if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous():
            raise TypeError('expected contiguous CUDA int64 tensor')


def _rows(t):
    """(ptr tensor, leading dim) of a 2-D row-major view (stride(1) == 1)."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f'need a 2-D tensor with unit inner stride, got {tuple(t.shape)} {t.stride()}')
    return t.stride(0)


GEMM_CFG_NAMES = ['64x64x32', '128x32x32', '128x64x32', '128x128x32', '128x64x64', '128x128x64',
                  '128x64x32w8', '128x64x64w8', '128x128x64w8']


def gemm_force_config(cfg):
    return _lib.load().t2h_gemm_force_config(int(cfg))


# ---- optional HIP-event profiling of GEMM launches (bench.py roofline leg) ----
_prof = None
# one sampled launch: events (e0, e1) around it; kind 'kernel' = the kernel's own start / end, 'stream' = kernel + launch
# boundary (split GEMM only, with its tile configuration cfg and, 'kernel', the phase-stamp buffer)
ProfRec = collections.namedtuple('ProfRec', 'label flops e0 e1 kind cfg stamps', defaults=(None, None, None))


def gemm_profile_start(every=1):
    """Bracket every `every`-th t2h_gemm_f32 launch with HIP events on the
    launch stream (torch's current stream)."""
    global _prof
    _prof = dict(every=max(1, int(every)), count=0, recs=[])


def gemm_profile_active():
    return _prof is not None


SPLIT_CFG_NAMES = {0: '128x64', 1: '128x128', 2: '64x64', 3: '128x64, 8 waves', 5: '128x256', 6: '128x64, 2 K groups',
                   8: '256x128, ping-pong LDS-DMA', 9: 'few rows (16x16 per workgroup, K over 8 waves)',
                   10: '128x192, ping-pong LDS-DMA', 11: '128x128, ping-pong LDS-DMA'}


def _probe_clock(buf):
    """(median main-loop time in us, median shader clock in GHz over the main loop) from a phase-stamp buffer of
    t2h_gemm_split_probe_next_launch; None if the launch left no stamps (few-rows kernel)."""
    t = buf.view(-1, 16).cpu()
    t = t[(t[:, 1] != 0) & (t[:, 2] != 0)].double()
    if t.shape[0] == 0:
        return None
    us = (t[:, 2] - t[:, 1]) * 0.01
    ghz = (t[:, 10] - t[:, 9]) / (us * 1e3)
    return float(us.median()), float(ghz.median())


def gemm_profile_stop():
    """-> {kernel label: dict(kernel, n, ms, flops, ...)} (synchronises).  The split GEMM appears once as
    'gemm_split_kernel<2xfp16>' (all instantiations, launch-weighted) and once per tile configuration of the
    dispatcher under that record's 'by_cfg'; records that carried a phase-stamp buffer add the main loop's
    duration and the shader clock it ran at."""
    global _prof
    p, _prof = _prof, None
    if not p:
        return {}
    torch.cuda.synchronize()
    out = {}

    def add(r, flops, e0, e1, kind, probe):
        if kind == 'stream':  # interval on the stream: kernel + launch boundary
            r['n_stream'] += 1
            r['ms_stream'] += e0.elapsed_time(e1)
            r['flops_stream'] += flops
            return
        r['kernel_timed'] = r['kernel_timed'] or kind == 'kernel'
        r['n'] += 1
        r['ms'] += e0.elapsed_time(e1)
        r['flops'] += flops
        if probe is not None:
            r['n_probe'] += 1
            r['loop_us'] += probe[0]
            r['loop_ghz'] += probe[1]

    blank = lambda label: dict(kernel=label, n=0, ms=0.0, flops=0.0, n_stream=0, ms_stream=0.0, flops_stream=0.0,
                               kernel_timed=False, n_probe=0, loop_us=0.0, loop_ghz=0.0)
    for label, flops, e0, e1, kind, cfg, stamps in p['recs']:
        probe = _probe_clock(stamps) if stamps is not None else None
        r = out.setdefault(label, blank(label))
        add(r, flops, e0, e1, kind, probe)
        if cfg is not None:
            name = f'gemm_split_kernel<{SPLIT_CFG_NAMES.get(cfg, cfg)}>'
            add(r.setdefault('by_cfg', {}).setdefault(name, blank(name)), flops, e0, e1, kind, probe)
    return out


def _sample_phase():
    """Counts a launch of a profiled family; -> its place in the sampling period (0: sampled), None: profiling is off."""
    if _prof is None:
        return None
    _prof['count'] += 1
    return _prof['count'] % _prof['every']


def _bracketed(fn, args, what, label, flops, kind=None, cfg=None):
    """The launch fn(*args, stream) between a pair of events on the stream, appended to the profile."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(fn(*args, _stream()), what)
    e1.record()
    _prof['recs'].append(ProfRec(label, flops, e0, e1, kind, cfg))


def _launch(fn, g, what, label, extra=()):
    """fn(&g, *extra, stream) of a t2h_gemm_args launch; every `every`-th one of a profiling run is bracketed with
    events and recorded under `label` (a string, or g -> string)."""
    args = (ctypes.byref(g), *extra)
    if _sample_phase() != 0:
        return check(fn(*args, _stream()), what)
    _bracketed(fn, args, what, label if isinstance(label, str) else label(g), 2.0 * g.M * g.N * g.K * max(1, g.batch))


def _gemm_label(g):
    cfg = _lib.load().t2h_gemm_tile_config(ctypes.byref(g))
    return f"gemm_kernel<{GEMM_CFG_NAMES[cfg]},amode={g.a_mode},pro={int(bool(g.pro_scale))},btrans={g.b_trans}>"


def _gemm_args(a, w, out, M, N, K, lda, ldb, ldc, bias=None, residual=None, act=ACT_NONE, alpha=1.0, res_pre=False):
    """t2h_gemm_args of one plain GEMM: out[M, N] = act(alpha * a @ w^T + bias) + residual (a tensor's leading
    dimension is given, not derived: the split-row operands have none)."""
    g = GemmArgs()
    g.A, g.B, g.C = a.data_ptr(), w.data_ptr(), out.data_ptr()
    g.bias = bias.data_ptr() if bias is not None else None
    g.residual = residual.data_ptr() if residual is not None else None
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = lda, ldb, ldc
    g.ldr = _rows(residual) if residual is not None else 0
    g.epi_act, g.alpha, g.res_pre, g.batch = act, alpha, int(res_pre), 1
    return g


_CONV_MODES = {'same': (1, 1, 0), 'up': (1, 1, 1), 'down': (2, 0, 0)}  # (stride, pad, nearest x2 first)


def _conv_args(g, mode, hin, win, cin, pad=None, pro=None, pro_act=PRO_NONE):
    """... as an implicit convolution over NHWC pixel rows (a_mode 1) -- mode: 'same' (stride 1 pad 1), 'up' (nearest
    x2 then same conv), 'down' (zero-pad right / bottom by 1, stride 2) --, pro = (scale, shift) [n_img, C] tables
    applied with pro_act while the operand is staged."""
    stride, mode_pad, ups = _CONV_MODES[mode]
    g.a_mode, g.stride, g.pad, g.ups = 1, stride, mode_pad if pad is None else pad, ups
    g.Hin, g.Win, g.Cin, g.Hout, g.Wout = hin, win, cin, (hin << ups) // stride, (win << ups) // stride
    if pro is not None:
        sc, sh = pro
        _chk_f32(sc, sh)
        g.pro_scale, g.pro_shift, g.pro_ld, g.pro_act = sc.data_ptr(), sh.data_ptr(), sc.shape[1], pro_act
    return g


def gemm(a, w, out=None, bias=None, residual=None, act=ACT_NONE, alpha=1.0, pro=None,
         b_trans=False):
    """out[M,N] = act(alpha * pro(a)[M,K] @ w[N,K]^T + bias) + residual.

    a, w, out, residual: 2-D views with unit inner stride (row stride free).
    pro = (scale[n_img,K], shift[n_img,K], rows_per_img, pro_act).
    b_trans: w is given as [K,N]."""
    _chk_f32(a, w, out, bias, residual)
    M, K = a.shape
    N = w.shape[1] if b_trans else w.shape[0]
    assert (w.shape[0] if b_trans else w.shape[1]) == K, (a.shape, w.shape)
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32)
    g = _gemm_args(a, w, out, M, N, K, _rows(a), _rows(w), _rows(out), bias, residual, act, alpha)
    g.b_trans = int(b_trans)
    if pro is not None:
        sc, sh, rows, pact = pro
        _chk_f32(sc, sh)
        g.pro_scale, g.pro_shift = sc.data_ptr(), sh.data_ptr()
        g.pro_rows, g.pro_ld, g.pro_act = rows, sc.shape[1], pact
    _launch(_lib.load().t2h_gemm_f32, g, 't2h_gemm_f32', _gemm_label)
    return out


def conv_split_ok(n_pix_per_img, mode='same', act=ACT_NONE):
    """Shapes t2h_conv_split_f32 serves: stride-1 convolutions whose images hold a multiple of
    128 pixels (a workgroup never straddles two images)."""
    return mode in ('same', 'up') and n_pix_per_img % 128 == 0 and act in (ACT_NONE, ACT_RELU)


def gn_apply_split(x, scale=None, shift=None, rows_per_img=0, act=PRO_NONE, out=None):
    """fp32 pixel rows x [rows, C] -> split rows of act(x * scale[img] + shift[img]) (GroupNorm apply
    + swish in one pass; scale None = plain split): the activation operand of conv_split."""
    _chk_f32(x, scale, shift)
    rows, C = x.shape
    if out is None:
        out = split_rows_empty(rows, C, x.device)
    check(_lib.load().t2h_gn_apply_split_f32(_p(x), _rows(x), _p(scale), _p(shift),
                                             scale.shape[1] if scale is not None else 0, _p(out), rows,
                                             rows_per_img, C, act, overflow_flag(), _stream()), 't2h_gn_apply_split_f32')
    return out


def conv_split(xs, w_split, n_img, hin, win, cin, cout, taps=9, out=None, bias=None, residual=None,
               act=ACT_NONE, mode='same', res_pre=False, gn_stats=False):
    """Stride-1 convolution (taps 9: 3x3 'same' or, mode 'up', 3x3 after nearest x2; taps 1: 1x1) of
    split-row activations xs [n_img*hin*win, cin/32, 2, 32] with split-row weights
    w_split [cout, taps*cin/32, 2, 32] on the fp16 matrix cores; fp32 rows out [M, cout]."""
    _chk_f32(out, bias, residual)
    assert mode in ('same', 'up') and taps in (1, 9)
    ups = 1 if mode == 'up' else 0
    hout, wout = hin << ups, win << ups
    M = n_img * hout * wout
    assert xs.numel() == n_img * hin * win * cin * 2 and w_split.numel() == cout * taps * cin * 2, \
        (tuple(xs.shape), tuple(w_split.shape), n_img, hin, win, cin, cout, taps)
    if out is None:
        out = torch.empty((M, cout), device=xs.device, dtype=torch.float32)
    g = _conv_args(_gemm_args(xs, w_split, out, M, cout, taps * cin, 0, 0, _rows(out), bias, residual, act,
                              res_pre=res_pre), mode, hin, win, cin, pad=1 if taps == 9 else 0)
    if gn_stats:
        _gn_part(g, out, n_img, hout * wout)
    _launch(_lib.load().t2h_conv_split_f32, g, 't2h_conv_split_f32', 'conv_split_kernel<2xfp16>')
    return out


def _gn_part(g, out, n_img, hw_out):
    """per-(image, 128-row tile, channel) fp64 (sum, sum of squares) of a convolution's output, written by its
    epilogue; attached to `out`: groupnorm_tables(out, ...) then only reduces these partials"""
    out._t2h_gn_part = torch.empty((n_img, hw_out // 128, 2, g.N), device=out.device, dtype=torch.float64)
    g.gn_part_out = out._t2h_gn_part.data_ptr()


def conv_halo_ok(n_img, hout, wout, cin, cout, mode='same'):
    """Shapes t2h_conv_halo_f32 serves AND is meant for: 3x3 'same' / nearest-x2 convolutions whose 16 x 16-pixel
    tiles x 128-channel column tiles give at least 32 workgroups PER IMAGE (a chunk of 8 images then gives every CU
    one: the decoders' levels from 64 x 32 / 512 channels up); the small levels keep the 128-pixel tiles of
    t2h_conv_split_f32.  Deliberately NOT a function of n_img: the two kernels sum K in different orders, and an
    image must not depend on how many neighbours it is decoded with (tests/test_gpu_edge_cases.py:
    test_decode_chunk_boundary_is_invisible compares bit for bit).  T2H_HALO_CONV=0 switches the kernel off, =2 uses
    it wherever it serves the shape (tests)."""
    knob = os.environ.get('T2H_HALO_CONV', '1')
    if knob == '0':
        return False
    served = mode in ('same', 'up') and hout % 16 == 0 and wout % 16 == 0 and cin % 32 == 0 and cout % 8 == 0 and cin <= 512
    # (the kernel addresses an image and the weights with 32-bit byte offsets: beyond 2 GiB per image the two-kernel
    # path serves the layer -- 4096 x 2048 pixels of 128 channels; the decoders' largest is 1024 x 512)
    served = served and hout * wout * cin * 4 < 2**31 and cout * 9 * cin * 4 < 2**31
    return served and (knob == '2' or (hout // 16) * (wout // 16) * ((cout + 127) // 128) >= 32)


def conv_halo(x, w_split, n_img, hin, win, cin, cout, out=None, bias=None, residual=None, mode='same', pro=None,
              gn_stats=False):
    """3x3 convolution (mode 'same', or 'up': after nearest x2) of fp32 NHWC rows x [n_img*hin*win, >= cin] with
    split-row weights w_split [cout, 9*cin/32, 2, 32]; pro = (scale, shift) [n_img, C] GroupNorm tables applied with
    swish while the operand is staged (None: plain convolution).  fp32 rows out [M, cout]; gn_stats as conv_split."""
    _chk_f32(x, out, bias, residual)
    assert mode in ('same', 'up')
    ups = 1 if mode == 'up' else 0
    hout, wout = hin << ups, win << ups
    M = n_img * hout * wout
    assert x.shape[0] == n_img * hin * win and x.shape[1] >= cin and w_split.numel() == cout * 9 * cin * 2, \
        (tuple(x.shape), tuple(w_split.shape), n_img, hin, win, cin, cout)
    if out is None:
        out = torch.empty((M, cout), device=x.device, dtype=torch.float32)
    g = _conv_args(_gemm_args(x, w_split, out, M, cout, 9 * cin, _rows(x), 0, _rows(out), bias, residual),
                   mode, hin, win, cin, pro=pro, pro_act=PRO_SWISH)
    if gn_stats:
        _gn_part(g, out, n_img, hout * wout)
    _launch(_lib.load().t2h_conv_halo_f32, g, 't2h_conv_halo_f32', 'conv_halo_kernel<2xfp16>', (overflow_flag(), ))
    return out


def bgemm(a, w, out, alpha=1.0, b_trans=False):
    """Batched: a [b,M,K], w [b,N,K] (or [b,K,N] if b_trans), out [b,M,N]; 3-D
    views with unit inner stride (batch / row strides free)."""
    _chk_f32(a, w, out)
    nb, M, K = a.shape
    N = w.shape[2] if b_trans else w.shape[1]
    assert a.stride(2) == 1 and w.stride(2) == 1 and out.stride(2) == 1
    g = _gemm_args(a, w, out, M, N, K, a.stride(1), w.stride(1), out.stride(1), alpha=alpha)
    g.strideA, g.strideB, g.strideC = a.stride(0), w.stride(0), out.stride(0)
    g.batch, g.b_trans = nb, int(b_trans)
    _launch(_lib.load().t2h_gemm_f32, g, 't2h_gemm_f32(batched)', _gemm_label)
    return out


def conv3x3(x, w, n_img, hin, win, cin, out=None, bias=None, residual=None, act=ACT_NONE,
            pro=None, mode='same', res_pre=False, ksplit=None):
    """3x3 convolution of an NHWC image held as pixel rows x [n_img*hin*win, >=cin]
    with packed weights w [Cout, 9*cin] ([tap][cin] order).

    mode: 'same' (stride 1 pad 1), 'up' (nearest x2 then same conv),
          'down' (zero-pad right/bottom by 1, stride 2).
    ksplit: K slices on their own workgroups (t2h_gemm_args.ksplit): None = the library's choice from the layer's
          geometry (few pixels per image: the deep UNet levels), 1 = one pass over K, n > 1 = n slices."""
    _chk_f32(x, w, out, bias, residual)
    if mode not in _CONV_MODES:
        raise ValueError(mode)
    stride, _, ups = _CONV_MODES[mode]
    M, N = n_img * ((hin << ups) // stride) * ((win << ups) // stride), w.shape[0]
    assert w.shape[1] == 9 * cin and x.shape[0] == n_img * hin * win
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    g = _conv_args(_gemm_args(x, w, out, M, N, 9 * cin, _rows(x), _rows(w), _rows(out), bias, residual, act,
                              res_pre=res_pre), mode, hin, win, cin, pro=pro[:2] if pro is not None else None,
                   pro_act=pro[2] if pro is not None else PRO_NONE)
    # few pixels per image (the deep UNet levels): K split across workgroups, partial tiles in a workspace of this
    # call (stream-ordered like every torch allocation); the slice count depends on the layer's geometry only
    if ksplit is None:
        g.splitk_ws = ctypes.c_void_p(1)  # (non-NULL: ask what the library would do with a workspace)
        ksplit = _lib.load().t2h_gemm_ksplit(ctypes.byref(g))
        g.splitk_ws = None
    if ksplit is not None and ksplit > 1:
        ws = torch.empty(ksplit * M * N, device=x.device, dtype=torch.float32)
        g.splitk_ws, g.splitk_ws_floats, g.ksplit = ws.data_ptr(), ws.numel(), int(ksplit)
    else:
        g.ksplit = 1
    _launch(_lib.load().t2h_gemm_f32, g, 't2h_gemm_f32(conv)', _gemm_label)
    return out


def conv3x3_small(x, w, n_img, h, wd, cin, bias=None, pro=None, out=None):
    """3x3 'same' convolution with <= 4 output channels (conv_out) on the vector ALU, exact fp32;
    pro = (scale[n_img, C], shift[n_img, C], pro_act) as for conv3x3."""
    _chk_f32(x, w, bias, out)
    cout = w.shape[0]
    assert w.shape[1] == 9 * cin and x.shape[0] == n_img * h * wd and w.is_contiguous()
    if out is None:
        out = torch.empty((n_img * h * wd, cout), device=x.device, dtype=torch.float32)
    sc, sh, pact = pro if pro is not None else (None, None, PRO_NONE)
    _chk_f32(sc, sh)
    check(_lib.load().t2h_conv3x3_small_f32(_p(x), _rows(x), _p(w), _p(bias), _p(sc), _p(sh),
                                            sc.shape[1] if sc is not None else 0, int(pact), _p(out), _rows(out), n_img, h,
                                            wd, cin, cout, _stream()), 't2h_conv3x3_small_f32')
    return out


def conv3x3_small_ok(cin, cout, mode):
    return mode == 'same' and cout <= 4 and cin % 32 == 0


def layernorm(x, gamma, beta, out=None, eps=1e-5):
    _chk_f32(x, gamma, beta, out)
    assert x.is_contiguous()
    rows, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(_lib.load().t2h_layernorm_f32(_p(x), _p(gamma), _p(beta), _p(out), rows, C, eps, _stream()),
          't2h_layernorm_f32')
    return out


def split_rows_empty(rows, C, device):
    """Uninitialised split-row buffer [rows][C/32][2][32] fp16 (as int16)."""
    return torch.empty((rows, C // 32, 2, 32), device=device, dtype=torch.int16)


SPLIT_LO_SCALE = 2048.0


def split_planes_host(x):
    """(hi, lo) fp16 planes of an fp32 tensor: x = hi + lo / 2048 (round-to-nearest-even,
    bit-identical to the device split)."""
    x = x.float()
    if x.numel() and float(x.abs().max()) >= 65504.0:
        raise ValueError('split rows carry fp16 planes: |x| must stay below 65504 '
                         f'(got {float(x.abs().max()):.3g}); use the exact-fp32 kernels (T2H_SPLIT_GEMM=0)')
    hi = x.half()
    lo = ((x - hi.float()) * SPLIT_LO_SCALE).half()
    return hi, lo


def unsplit_rows_host(s, rows, C):
    """split rows (int16 view, any device) -> fp32 [rows, C] on the CPU"""
    pl = s.cpu().view(torch.float16).view(rows, C // 32, 2, 32).float()
    return (pl[:, :, 0] + pl[:, :, 1] / SPLIT_LO_SCALE).reshape(rows, C)


def split_rows(x, out=None):
    """fp32 x [rows, C] (unit inner stride) -> split rows (x = hi + lo / 2048, fp16 planes)."""
    _chk_f32(x)
    rows, C = x.shape
    if out is None:
        out = split_rows_empty(rows, C, x.device)
    check(_lib.load().t2h_split_rows_f32(_p(x), _rows(x), _p(out), rows, C, overflow_flag(), _stream()),
          't2h_split_rows_f32')
    return out


def pack_split_rows_host(w):
    """Host-side (torch CPU) repack of an fp32 matrix [N, K] into split rows."""
    hi, lo = split_planes_host(w)
    n, k = w.shape
    planes = torch.stack([hi, lo], 0).view(2, n, k // 32, 32).permute(1, 2, 0, 3).contiguous()
    return planes.view(torch.int16)


X8_TARGET_MAX = 32.0  # a tensor's calibration maximum is scaled into [16, 32): 14x headroom below e4m3's 448
X8_SCALE_MIN, X8_SCALE_MAX = 2.0 ** -7, 2.0 ** 22  # the domain of an x8 tensor's scale


def x8_scale_for(max_abs, target=X8_TARGET_MAX):
    """The power of two s with max_abs * s in [target / 2, target): the scale of a tensor's 8-bit planes (x8 format,
    csrc/common.h).  Weights use target 256 (their maximum is known exactly when they are packed)."""
    import math
    m = float(max_abs)
    if not (m > 0.0) or not math.isfinite(m):
        return 1.0
    # (never below 2^-7: 448 / s then stays under fp16's 65504, so a value the 8-bit planes can hold never overflows
    # the fp16 hi plane first.  Never above 2^22: where the fp16 hi plane is subnormal the residual l = (x - h) 2048 is
    # bounded by half a subnormal step, 2^-25 2048 = 2^-14, not by |h| -- l s <= 256 stays inside the 8-bit planes'
    # 448 for every fp32 x, which the producers' range test |x| s >= 448 alone would not notice)
    return min(max(2.0 ** (math.ceil(math.log2(target / m)) - 1), X8_SCALE_MIN), X8_SCALE_MAX)


def _chk_x8_scale(scale, what):
    s = float(scale)
    if not s <= X8_SCALE_MAX:
        raise ValueError(f'{what}: x8 scale {s:g} is above 2^22: the residual plane of values whose fp16 plane is '
                         'subnormal would leave the 8-bit range unflagged (ops.x8_scale_for caps the scale there)')
    return s


def absmax_f32(x, out_bits):
    """atomicMax of the fp32 bits of max |x| into out_bits[0] (int32 / uint32 device word the caller zeroed)."""
    _chk_f32(x)
    rows, C = x.shape
    check(_lib.load().t2h_absmax_f32(_p(x), _rows(x), rows, C, _p(out_bits), _stream()), 't2h_absmax_f32')


def split_rows_absmax(rows_split, rows, C, out_bits):
    """The same over the fp16 hi plane of split rows / x8 rows."""
    check(_lib.load().t2h_split_rows_absmax(_p(rows_split), rows, C, _p(out_bits), _stream()), 't2h_split_rows_absmax')


def split_rows_x8(x, scale, out=None):
    """fp32 x [rows, C] -> x8 rows [rows][C/32][hi16 | hi8 | lo8] (same byte size as split rows), 8-bit planes
    scaled by the power of two `scale`."""
    scale = _chk_x8_scale(scale, 'split_rows_x8')
    _chk_f32(x)
    rows, C = x.shape
    if out is None:
        out = split_rows_empty(rows, C, x.device)
    check(_lib.load().t2h_split_rows_x8_f32(_p(x), _rows(x), _p(out), rows, C, scale, overflow_flag(), _stream()),
          't2h_split_rows_x8_f32')
    return out


def unpack_x8_rows_host(s, rows, C, scale):
    """x8 rows (int16 view, any device) -> (hi fp32 [rows, C], hi8 / scale, lo8 / scale) on the CPU: the three planes
    as the numbers they stand for (tests)."""
    raw = s.cpu().contiguous().view(torch.uint8).view(rows, C // 32, 128)
    hi = raw[:, :, :64].contiguous().view(torch.float16).float().reshape(rows, C)
    h8 = raw[:, :, 64:96].contiguous().view(torch.float8_e4m3fn).float().reshape(rows, C) / scale
    l8 = raw[:, :, 96:].contiguous().view(torch.float8_e4m3fn).float().reshape(rows, C) / scale
    return hi, h8, l8


def layernorm_x8(x, gamma, beta, out_x8, scale, eps=1e-5):
    """LayerNorm whose result is written in the x8 format."""
    scale = _chk_x8_scale(scale, 'layernorm_x8')
    _chk_f32(x, gamma, beta)
    assert x.is_contiguous()
    rows, C = x.shape
    check(_lib.load().t2h_layernorm_x8_f32(_p(x), _p(gamma), _p(beta), _p(out_x8), rows, C, eps, scale,
                                           overflow_flag(), _stream()), 't2h_layernorm_x8_f32')
    return out_x8


def mha_split_auto_form(B, T, n_head):
    """the form (1 all keys / 2 key halves) mha_split / mha_split_x8 pick by themselves for B samples (t2h_mha_split_form)"""
    form = _lib.load().t2h_mha_split_form(int(B), int(T), int(n_head))
    if form not in (1, 2):
        check(1, 't2h_mha_split_form')
    return form


class mha_split_form:
    """`with mha_split_form(2):` -- mha_split / mha_split_x8 of this thread run on that form (1 all keys, 2 key halves)
    instead of the one picked from the batch size (t2h_mha_split_force_form); None: nothing is forced."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        if self.form is not None:
            self.old = _lib.load().t2h_mha_split_force_form(int(self.form))

    def __exit__(self, *exc):
        if self.form is not None:
            _lib.load().t2h_mha_split_force_form(self.old)


def mha_split_x8(qk_split, ld_cols, vt, B, T, n_head, out_x8, scale):
    """mha_split with the output written in the x8 format."""
    scale = _chk_x8_scale(scale, 'mha_split_x8')
    check(_lib.load().t2h_mha_split_x8_f32(_p(qk_split), ld_cols, _p(vt), _p(out_x8), scale, B, T, n_head,
                                           overflow_flag(), _stream()), 't2h_mha_split_x8_f32')
    return out_x8


def gemm_split(a_split, w_split, M, N, K, out=None, out_split=None, bias=None, residual=None, act=ACT_NONE,
               vt=None, vt_col0=0, vt_T=0, vt_hd=64, x8=None, out_x8_scale=None, ksplit=0, cfg_rows=0):
    """C = act(A @ W^T + bias) + residual on the fp16 matrix cores at fp32-class
    accuracy; a_split / w_split are split rows.  Writes fp32 `out` and / or the
    split-row form `out_split` of the result.  With `vt` the output columns from
    `vt_col0` on go to the transposed value planes of mha_split instead
    (t2h_gemm_split_args.Vt).
    x8 = (scale_A, scale_B): the operands are x8 rows (fp16 plane + two e4m3 planes scaled by those powers of two),
    the cross terms run on the 8-bit matrix instruction; out_x8_scale: `out_split` is written in the x8 format.
    cfg_rows > 0: the tile configuration of a problem of that many rows (t2h_gemm_split_args.cfg_rows) -- a row's bits
    then do not depend on M."""
    _chk_f32(out, bias, residual)
    g = _lib.GemmSplitArgs()
    g.cfg_rows = int(cfg_rows)
    if x8 is not None:
        g.fmt = 1
        g.lo_mul = 1.0 / (SPLIT_LO_SCALE * float(x8[0]) * float(x8[1]))
    if out_x8_scale is not None:
        g.out_fmt, g.out_scale = 1, _chk_x8_scale(out_x8_scale, 'gemm_split(out_x8_scale=)')
    g.ksplit = int(ksplit)  # (> 1: `out` holds ksplit * M rows of partial tiles; experiment, t2h_hip.h)
    g.A, g.B = a_split.data_ptr(), w_split.data_ptr()
    g.C = out.data_ptr() if out is not None else None
    g.C_split = out_split.data_ptr() if out_split is not None else None
    g.bias = bias.data_ptr() if bias is not None else None
    g.residual = residual.data_ptr() if residual is not None else None
    g.M, g.N, g.K = M, N, K
    g.ldc = _rows(out) if out is not None else 0
    g.ldr = _rows(residual) if residual is not None else 0
    g.epi_act = act
    if vt is not None:
        g.Vt, g.vt_col0, g.vt_T, g.vt_hd = vt.data_ptr(), vt_col0, vt_T, vt_hd
    if out_split is not None or vt is not None:
        g.overflow_flag = _ovf_slot()[0].data_ptr()
    lib = _lib.load()
    phase = _sample_phase()
    # algorithmic (fp32-equivalent) FLOPs; the kernel issues 3 fp16 products per multiply.  Two kinds of
    # samples, on DIFFERENT launches (timing a kernel through hipExtLaunchKernelGGL adds packets around it):
    if phase is not None and phase in (0, _prof['every'] // 2):
        cfg = lib.t2h_gemm_split_tile_config(ctypes.byref(g))
        if phase != 0:
            # events recorded on the stream around the launch, which so run from the end of the previous
            # kernel: kernel + dependent-launch boundary
            _bracketed(lib.t2h_gemm_split_f32, (ctypes.byref(g), ), 't2h_gemm_split_f32', _split_label(g),
                       2.0 * M * N * K, 'stream', cfg)
            return out if out is not None else out_split
        # (k0, k1) receive the kernel's OWN start / end (t2h_gemm_split_time_next_launch): kernel time; the same
        # launch stores its phase stamps (main loop duration + the shader clock it ran at)
        k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        k0.record()  # (creates the hipEvent_t handles the hook hands to the launch)
        k1.record()
        # (sized for the smallest tile any configuration uses, 64 x 64: the kernel stores 16 words per workgroup unbounded)
        stamps = torch.zeros(16 * (-(-M // 64)) * (-(-N // 64)), dtype=torch.int64, device=a_split.device)
        check(lib.t2h_gemm_split_time_next_launch(ctypes.c_void_p(k0.cuda_event), ctypes.c_void_p(k1.cuda_event)),
              't2h_gemm_split_time_next_launch')
        check(lib.t2h_gemm_split_probe_next_launch(_p(stamps)), 't2h_gemm_split_probe_next_launch')
        _prof['recs'].append(ProfRec(_split_label(g), 2.0 * M * N * K, k0, k1, 'kernel', cfg, stamps))
    check(lib.t2h_gemm_split_f32(ctypes.byref(g), _stream()), 't2h_gemm_split_f32')
    return out if out is not None else out_split


def _split_label(g):
    """profile label of a split-GEMM launch: '<2xfp16>' = three fp16 partial products, '<x8>' = fp16 hi*hi + both
    cross terms in one 8-bit instruction"""
    return 'gemm_split_kernel<x8>' if g.fmt == 1 else 'gemm_split_kernel<2xfp16>'


def split_overflow_async(reset=True):
    """Enqueues the read-back (and optional clear) of the current stream's overflow word; -> the pinned host
    tensor the value lands in, valid once the stream has been synchronised.  No host wait here."""
    flag, host = _ovf_slot()
    check(_lib.load().t2h_split_overflow_async(_p(flag), _p(host), int(bool(reset)), _stream()), 't2h_split_overflow_async')
    return host


def split_overflow_bits(reset=True):
    """The sticky overflow word of the current stream's split-row producers since the last reset (include/t2h_hip.h):
    bit 0: a value outside fp16's range (|x| >= 65504); bit 1: a value outside the 8-bit planes' range of an x8
    tensor (|x| s >= 448).  Synchronises the current stream -- here, in the host code, not inside the library."""
    host = split_overflow_async(reset)
    torch.cuda.current_stream().synchronize()
    return int(host[0])


def split_overflow(reset=True):
    """True if any split-row producer flagged a value since the last reset (any bit of split_overflow_bits)."""
    return bool(split_overflow_bits(reset))


def vt_empty(B, n_head, T, device, hd=64):
    """Transposed value planes [B][H][2][hd][T] fp16 (as int16) for mha_split."""
    return torch.empty(B, n_head, 2, hd, T, dtype=torch.int16, device=device)


def vt_key_positions(T):
    """Position of key k inside the Vt planes (include/t2h_hip.h, t2h_gemm_split_args.Vt)."""
    k = torch.arange(T)
    w = k & 31
    return (k & ~31) + 16 * (w >> 4) + 8 * ((w >> 2) & 1) + 4 * ((w >> 3) & 1) + (w & 3)


def mha_split(qk_split, ld_cols, vt, B, T, n_head, out=None, out_split=None):
    """Attention with q, k read as split rows and v as transposed planes; both
    products as three fp16 partial products (fp32-class accuracy)."""
    _chk_f32(out)
    check(_lib.load().t2h_mha_split_f32(_p(qk_split), ld_cols, _p(vt), _p(out) if out is not None else None,
                                        _p(out_split) if out_split is not None else None, B, T, n_head,
                                        overflow_flag() if out_split is not None else None, _stream()), 't2h_mha_split_f32')
    return out if out is not None else out_split


def layernorm_split(x, gamma, beta, out_split, eps=1e-5):
    """LayerNorm whose result is written as split rows."""
    _chk_f32(x, gamma, beta)
    assert x.is_contiguous()
    rows, C = x.shape
    check(_lib.load().t2h_layernorm_split_f32(_p(x), _p(gamma), _p(beta), _p(out_split), rows, C, eps,
                                              overflow_flag(), _stream()), 't2h_layernorm_split_f32')
    return out_split


def mha_noncausal_split(qkv, B, T, n_head, out_split):
    """Attention whose output is written as split rows."""
    _chk_f32(qkv)
    assert qkv.is_contiguous() and qkv.shape == (B * T, 3 * n_head * 64)
    check(_lib.load().t2h_mha_noncausal_split_f32(_p(qkv), _p(out_split), B, T, n_head, overflow_flag(), _stream()),
          't2h_mha_noncausal_split_f32')
    return out_split


def groupnorm_tables(x, gamma, beta, n_img, hw, groups=32, eps=1e-6):
    """GroupNorm statistics of x [n_img*hw, C] -> (scale, shift) [n_img, C]."""
    _chk_f32(x, gamma, beta)
    C = gamma.shape[0]
    lib = _lib.load()
    scale = torch.empty((n_img, C), device=x.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    part = getattr(x, '_t2h_gn_part', None)
    if part is not None and tuple(part.shape[:1] + part.shape[2:]) == (n_img, 2, C) and x.shape[0] == n_img * hw:
        # the producing conv already left per-tile partial sums: no pass over x
        check(lib.t2h_groupnorm_finalize_f32(_p(part), part.shape[1], _p(gamma), _p(beta), _p(scale), _p(shift),
                                             n_img, hw, C, groups, eps, _stream()), 't2h_groupnorm_finalize_f32')
        return scale, shift
    ws = torch.empty(lib.t2h_groupnorm_workspace_bytes(n_img, hw, C) // 8, device=x.device,
                     dtype=torch.float64)
    check(lib.t2h_groupnorm_tables_f32(_p(x), _rows(x), _p(gamma), _p(beta), _p(scale), _p(shift),
                                       n_img, hw, C, groups, eps, _p(ws), _stream()),
          't2h_groupnorm_tables_f32')
    return scale, shift


def spatial_attention(qkv, n_img, n, c, out=None):
    """AttnBlock attention without the N x N tensor: qkv rows [n_img * n, 3c] (q | k | v) -> rows [n_img * n, c]."""
    _chk_f32(qkv, out)
    assert qkv.shape == (n_img * n, 3 * c) and c in (256, 512) and n % 32 == 0
    if out is None:
        out = torch.empty((n_img * n, c), device=qkv.device, dtype=torch.float32)
    check(_lib.load().t2h_spatial_attention_f32(_p(qkv), _rows(qkv), _p(out), _rows(out), n_img, n, c, float(int(c)**(-0.5)),
                                                _stream()), 't2h_spatial_attention_f32')
    return out


def spatial_attention_ok(n, c):
    return c in (256, 512) and n % 32 == 0


def softmax_rows_(x):
    _chk_f32(x)
    x2 = x.view(-1, x.shape[-1])
    check(_lib.load().t2h_softmax_rows_f32(_p(x2), x2.shape[0], x2.shape[1], x2.stride(0), _stream()),
          't2h_softmax_rows_f32')
    return x


def embed_sum4(idx, segm, tex, tok_emb, pos_emb, segm_emb, tex_emb, out=None):
    _chk_i64(idx, segm, tex)
    _chk_f32(tok_emb, pos_emb, segm_emb, tex_emb, out)
    B, T = idx.shape
    C = tok_emb.shape[1]
    if out is None:
        out = torch.empty((B * T, C), device=idx.device, dtype=torch.float32)
    check(_lib.load().t2h_embed_sum4_f32(_p(idx), _p(segm), _p(tex), _p(tok_emb), _p(pos_emb),
                                         _p(segm_emb), _p(tex_emb), _p(out), B, T, C, _stream()),
          't2h_embed_sum4_f32')
    return out


def mha_noncausal(qkv, B, T, n_head, out=None):
    _chk_f32(qkv, out)
    assert qkv.is_contiguous() and qkv.shape == (B * T, 3 * n_head * 64)
    if out is None:
        out = torch.empty((B * T, n_head * 64), device=qkv.device, dtype=torch.float32)
    check(_lib.load().t2h_mha_noncausal_f32(_p(qkv), _p(out), B, T, n_head, _stream()),
          't2h_mha_noncausal_f32')
    return out


def unmask_step(rand, t, unmasked, changes, tex, head_count, changed_rows=None, n_heads=0):
    """head_count: int32 [n_heads (+1)]; with changed_rows (int32 [n]) the changed rows are
    appended to it and counted in head_count[n_heads]."""
    _chk_f32(rand)
    n = rand.numel()
    if changed_rows is not None:
        assert changed_rows.dtype == torch.int32 and changed_rows.numel() >= n
        assert head_count.numel() > n_heads
    check(_lib.load().t2h_unmask_step(_p(rand), int(t), _p(unmasked), _p(changes), _p(tex),
                                      _p(head_count), n, _p(changed_rows), int(n_heads), _stream()),
          't2h_unmask_step')


def torch_draw_geometry(numel, device=None):
    """(threads of the grid ATen launches for an elementwise random draw of `numel` floats, generator
    offset increment of that draw) -- calc_execution_policy of ATen/native/cuda/DistributionTemplates.h:
    block 256, grid = min(#CU * (max threads per CU / 256), ceil(numel / 256)), unroll 4."""
    prop = torch.cuda.get_device_properties(device if device is not None else torch.cuda.current_device())
    grid = min(prop.multi_processor_count * (prop.max_threads_per_multi_processor // 256), (numel + 255) // 256)
    return 256 * grid, ((numel - 1) // (256 * grid * 4) + 1) * 4


def philox_exponential(seed, offset, numel, device):
    """What `torch.empty(numel, device=device).exponential_()` returns on a generator with this seed /
    offset, computed element by element (t2h_philox_exponential_f32)."""
    out = torch.empty(numel, device=device, dtype=torch.float32)
    gt, _ = torch_draw_geometry(numel, device)
    check(_lib.load().t2h_philox_exponential_f32(int(seed), int(offset), gt, _p(out), numel, _stream()),
          't2h_philox_exponential_f32')
    return out


def philox_uniform(seed, offset, numel, device):
    """What `torch.rand(numel, device=device)` returns on a generator with this seed / offset
    (t2h_philox_uniform_f32)."""
    out = torch.empty(numel, device=device, dtype=torch.float32)
    gt, _ = torch_draw_geometry(numel, device)
    check(_lib.load().t2h_philox_uniform_f32(int(seed), int(offset), gt, _p(out), numel, _stream()),
          't2h_philox_uniform_f32')
    return out


def seeds_tensor(seeds, device):
    """validated per-image seeds (options.image_seeds: Python ints in [0, 2^64)) -> int64 [B] on the device holding the
    same bits (the kernels read the words back as uint64)"""
    return torch.tensor([schedule.as_int64(s) for s in seeds], dtype=torch.int64).to(device)


def unmask_schedule(seed, offset, tex, steps, n_heads, n_class, keep=None, seeds=None):
    """The whole unmasking schedule of a sampling run on torch's device generator (seed, offset before
    the first draw) in one launch (t2h_unmask_schedule).  tex int64 [n]; keep uint8 [n] (region editing,
    t2h_unmask_schedule_keep): rows that start unmasked (step 0, never drawn).  Returns
    (step_of_row int32 [n], head_mask int32 [steps + 1], rand_inc, expo_inc) -- device tensors.
    seeds (per-image seeds; `seed` / `offset` are then not read): one integer in [0, 2^64) per image,
    validated here before the launch (options.image_seeds) -- image b of the n / B rows each gets the schedule of the
    call on its rows alone with seed seeds[b] at offset 0 (t2h_unmask_schedule_batch); head_mask is [B, steps + 1] and
    the increments are those of ONE image's draws."""
    _chk_i64(tex)
    n = tex.numel()
    dev = tex.device
    if seeds is not None:
        if not options.is_per_image(seeds) or len(seeds) < 1 or n % len(seeds) != 0:
            raise ValueError(f'seeds: one integer per image expected, dividing the {n} token rows, got {seeds!r}')
        B = len(seeds)
        seeds = options.image_seeds(B, seeds)
        T = n // B
        rand_gt, rand_inc = torch_draw_geometry(T, dev)
        _, expo_inc = torch_draw_geometry(T * n_class, dev)
        if keep is not None:
            _chk_u8(keep, n)
        seeds_dev = seeds_tensor(seeds, dev)
        step_of_row = torch.empty(n, dtype=torch.int32, device=dev)
        head_mask = torch.empty((B, steps + 1), dtype=torch.int32, device=dev)
        check(_lib.load().t2h_unmask_schedule_batch(_p(seeds_dev), rand_gt, rand_inc, expo_inc, _p(tex), _p(keep), B, T,
                                                    int(steps), int(n_heads), _p(step_of_row), _p(head_mask), _stream()),
              't2h_unmask_schedule_batch')
        return step_of_row, head_mask, rand_inc, expo_inc
    rand_gt, rand_inc = torch_draw_geometry(n, dev)
    _, expo_inc = torch_draw_geometry(n * n_class, dev)
    step_of_row = torch.empty(n, dtype=torch.int32, device=dev)
    head_mask = torch.empty(steps + 1, dtype=torch.int32, device=dev)
    if keep is not None:
        _chk_u8(keep, n)
        check(_lib.load().t2h_unmask_schedule_keep(int(seed), int(offset), rand_gt, rand_inc, expo_inc, _p(tex),
                                                   _p(keep), n, int(steps), int(n_heads), _p(step_of_row),
                                                   _p(head_mask), _stream()), 't2h_unmask_schedule_keep')
        return step_of_row, head_mask, rand_inc, expo_inc
    check(_lib.load().t2h_unmask_schedule(int(seed), int(offset), rand_gt, rand_inc, expo_inc, _p(tex), n, int(steps),
                                          int(n_heads), _p(step_of_row), _p(head_mask), _stream()),
          't2h_unmask_schedule')
    return step_of_row, head_mask, rand_inc, expo_inc


def _chk_u8(t, n):
    if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.numel() != n:
        raise TypeError(f'expected a contiguous CUDA uint8 tensor of {n} elements, got {t.dtype} {tuple(t.shape)}')


def edit_prefill(src_lists, tex, keep, mask_id, n_class, x_t=None, out=None, err=None):
    """Initial state of a region edit (t2h_edit_prefill): src_lists int64 [n_heads, n], tex int64 [n], keep uint8 [n]
    -> x_t [n] (kept rows: their source token, the rest mask_id) and out [n_heads, n] (the kept tokens, -1 elsewhere),
    each written only if given.  err: uint32-sized int32 word [1] (zeroed here); after the launch it holds n - (first
    kept row without a valid source token), 0 if there is none.  Returns err."""
    _chk_i64(src_lists, tex)
    n_heads, n = src_lists.shape
    assert src_lists.is_contiguous() and tex.numel() == n
    _chk_u8(keep, n)
    if x_t is not None:
        assert x_t.dtype == torch.int64 and x_t.is_contiguous() and x_t.numel() == n
    if out is not None:
        assert out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (n_heads, n)
    if err is None:
        err = torch.empty(1, dtype=torch.int32, device=src_lists.device)
    err.zero_()
    check(_lib.load().t2h_edit_prefill(_p(src_lists), _p(tex), _p(keep), int(mask_id), _p(x_t), _p(out), _p(err), n,
                                       n_heads, int(n_class), _stream()), 't2h_edit_prefill')
    return err


def region_keep(B, H, W, cells, mask=None, parsing=None, labels=None):
    """Token rows an edit keeps (t2h_region_keep) -> uint8 [B, th * tw]: 0 iff any pixel of the row's cell is in the
    region.  mask: uint8 / bool / fp32 [B, 1, H, W] (nonzero = region) or parsing: fp32 [B, 1, H, W] class ids with
    labels: iterable of ids in [0, 64)."""
    th, tw = cells
    keep = torch.empty((B, th * tw), dtype=torch.uint8, device=(mask if mask is not None else parsing).device)
    if mask is not None:
        assert mask.is_contiguous() and mask.numel() == B * H * W
        if mask.dtype in (torch.uint8, torch.bool):
            mode, m8, mf = 0, mask.view(torch.uint8), None
        elif mask.dtype == torch.float32:
            mode, m8, mf = 1, None, mask
        else:
            raise TypeError(f'region mask must be uint8, bool or float32, got {mask.dtype}')
        bits = 0
    else:
        _chk_f32(parsing)
        assert parsing.is_contiguous() and parsing.numel() == B * H * W
        mode, m8, mf = 2, None, parsing
        bits = 0
        for lb in labels:
            if not 0 <= int(lb) < 64:
                raise ValueError(f'label ids must lie in [0, 64), got {lb}')
            bits |= 1 << int(lb)
    check(_lib.load().t2h_region_keep(_p(m8), _p(mf), bits, mode, B, H, W, th, tw, _p(keep), _stream()),
          't2h_region_keep')
    return keep


def merge_kept_indices(src_lists, keep, dst_lists):
    """dst_lists[:, r] = src_lists[:, r] where keep[r] (t2h_merge_kept_indices, in place; [n_heads, n] int64)."""
    _chk_i64(src_lists, dst_lists)
    n_heads, n = dst_lists.shape
    assert src_lists.is_contiguous() and dst_lists.is_contiguous() and tuple(src_lists.shape) == (n_heads, n)
    _chk_u8(keep, n)
    check(_lib.load().t2h_merge_kept_indices(_p(src_lists), _p(keep), _p(dst_lists), n, n_heads, _stream()),
          't2h_merge_kept_indices')
    return dst_lists


def fold_keep(folds, B, cells, keep=None, device=None):
    """The K keep masks of the pseudo-likelihood critic (t2h_fold_keep) -> uint8 [K, B, th * tw]: 1 iff
    the row is not in fold k or the caller keeps it (keep: uint8 [B * th * tw] or None).  folds: options.REVISE_FOLDS."""
    th, tw = cells
    folds = options.revise_folds_value(folds)
    n = int(B) * th * tw
    if keep is not None:
        _chk_u8(keep, n)
        device = keep.device
    keep_k = torch.empty((int(folds), int(B), th * tw), dtype=torch.uint8, device=device)
    check(_lib.load().t2h_fold_keep(_p(keep), int(folds), int(B), th, tw, _p(keep_k), _stream()), 't2h_fold_keep')
    return keep_k


def fold_gather(logp_k, folds, B, cells, rank_k=None):
    """Every row from the evaluation that hid it (t2h_fold_gather): logp_k f32 [K, B * T] (rank_k int32 likewise, or
    None) -> logp f32 [B * T] (, rank int32 [B * T])."""
    th, tw = cells
    n = int(B) * th * tw
    _chk_f32(logp_k)
    assert logp_k.is_contiguous() and logp_k.numel() == int(folds) * n
    logp = torch.empty(n, dtype=torch.float32, device=logp_k.device)
    rank = None
    if rank_k is not None:
        assert rank_k.dtype == torch.int32 and rank_k.is_contiguous() and rank_k.numel() == int(folds) * n
        rank = torch.empty(n, dtype=torch.int32, device=logp_k.device)
    check(_lib.load().t2h_fold_gather(_p(logp_k), _p(rank_k), int(folds), int(B), th, tw, _p(logp), _p(rank), _stream()),
          't2h_fold_gather')
    return logp if rank is None else (logp, rank)


def select_lowest(score, count):
    """The rows to redo (t2h_select_lowest): score f32 [B, T] (NaN = not eligible), count int32 [B] -> (keep_out uint8
    [B, T]: 0 for the min(count[b], eligible_b) lowest-scored rows of image b -- ties to the lower row --, 1 elsewhere;
    n_sel int32 [B]).  Nothing is read back."""
    _chk_f32(score)
    B, T = score.shape
    assert score.is_contiguous() and count.dtype == torch.int32 and count.is_cuda and count.numel() == B
    keep_out = torch.empty((B, T), dtype=torch.uint8, device=score.device)
    n_sel = torch.empty(B, dtype=torch.int32, device=score.device)
    check(_lib.load().t2h_select_lowest(_p(score), _p(count), B, T, _p(keep_out), _p(n_sel), _stream()),
          't2h_select_lowest')
    return keep_out, n_sel


def accept_merge(cand_lists, cand_score, sum_cand, cur_lists, cur_score, sum_cur, B, always=False):
    """Per-image accept (t2h_accept_merge, in place on cur_lists int64 [n_heads, B * T] / cur_score f32 [B * T]): image
    b takes the candidate's lists and scores iff always or sum_cand[b] > sum_cur[b] -> (sum_out f32 [B], accepted uint8
    [B])."""
    _chk_i64(cand_lists, cur_lists)
    _chk_f32(cand_score, cur_score, sum_cand, sum_cur)
    n_heads, n = cur_lists.shape
    B = int(B)
    assert tuple(cand_lists.shape) == (n_heads, n) and n % B == 0 and cand_score.numel() == n == cur_score.numel()
    assert cand_score.is_contiguous() and cur_score.is_contiguous() and sum_cand.numel() == B == sum_cur.numel()
    sum_out = torch.empty(B, dtype=torch.float32, device=cur_lists.device)
    accepted = torch.empty(B, dtype=torch.uint8, device=cur_lists.device)
    check(_lib.load().t2h_accept_merge(_p(cand_lists), _p(cand_score), _p(sum_cand), _p(sum_cur), int(bool(always)),
                                       _p(cur_lists), _p(cur_score), _p(sum_out), _p(accepted), B, n // B, n_heads,
                                       _stream()), 't2h_accept_merge')
    return sum_out, accepted


def schedule_advance(rows_tbl, aux64_tbl, aux32_tbl, round_ctr, cur_rows, cur_aux64, cur_aux32, maxr):
    """Round cursor (t2h_schedule_advance): cur_* <- round *round_ctr of the padded tables; *round_ctr += 1."""
    check(_lib.load().t2h_schedule_advance(_p(rows_tbl), _p(aux64_tbl), _p(aux32_tbl), _p(round_ctr), _p(cur_rows),
                                           _p(cur_aux64), _p(cur_aux32), int(maxr), _stream()), 't2h_schedule_advance')


def gather_rows(src, rows, n_rows, out=None):
    """out[i] = src[rows[i]] (rows int32 on the device, first n_rows used); src 2-D+ contiguous, any dtype
    whose row is a multiple of 16 bytes."""
    assert src.is_contiguous() and rows.dtype == torch.int32
    row_bytes = src[0].numel() * src.element_size()
    if out is None:
        out = torch.empty((int(n_rows), ) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    check(_lib.load().t2h_gather_rows(_p(src), _p(rows), _p(out), int(n_rows), row_bytes, _stream()), 't2h_gather_rows')
    return out


# (top_k, top_p) -> the validated (top_k, top_p_q) pair of the C structs: ONE helper, shared with the option surface
TOP_P_ONE = options.TOP_P_ONE
truncation_settings = options.truncation_settings


# ---- per-image sampling controls ("Per-image sampling controls")
SAMPLE_PARAMS_DTYPE = np.dtype([('temp', '<f4'), ('top_k', '<i4'), ('top_p_q', '<u4')])  # struct t2h_sample_params
assert SAMPLE_PARAMS_DTYPE.itemsize == ctypes.sizeof(_lib.SampleParams) == 12

# scalar controls: temp as given, trunc = truncation_settings' pair, table None (today's launches); per image: table =
# SAMPLE_PARAMS_DTYPE [B] in the CALLER's sample order (the engine permutes it with the batch), temp / trunc None
SamplingParams = collections.namedtuple('SamplingParams', 'temp trunc table')


def sampling_params(batch, temp=1.0, top_k=None, top_p=None, n_class=None, per_image=False):
    """The draw controls of one sampling call, validated on the host (ValueError; nothing has been drawn or launched):
    all scalars -> SamplingParams(temp, truncation_settings(top_k, top_p, n_class), None), exactly what the scalar
    path always used.  If any of the three is a sequence with one entry per image (options.per_image_values), or
    per_image is set (a per-image control of another kind: rounds, choice_temp), -> the table of t2h_sample_params,
    scalars repeated for every image.  Entry b must be what the scalar accepts (temp > 0; truncation_settings); an
    error names the image.  A sequence whose entries are all equal stays a table."""
    seqs = [options.per_image_values(batch, v, what) for v, what in ((temp, 'temp'), (top_k, 'top_k'), (top_p, 'top_p'))]
    if all(s is None for s in seqs) and not per_image:
        return SamplingParams(temp, truncation_settings(top_k, top_p, n_class), None)
    temps, ks, ps = (s if s is not None else [v] * int(batch) for s, v in zip(seqs, (temp, top_k, top_p)))
    table = np.zeros(int(batch), dtype=SAMPLE_PARAMS_DTYPE)
    for b in range(int(batch)):
        t = temps[b]
        if isinstance(t, bool) or not isinstance(t, numbers.Real) or not float(t) > 0.0 or float(t) == float('inf'):
            raise ValueError(f'image {b}: temp must be a finite number > 0, got {t!r}')
        try:
            k, p_q = truncation_settings(ks[b], ps[b], n_class)
        except ValueError as e:
            raise ValueError(f'image {b}: {e}') from None
        table[b] = (float(t), k, p_q)
    return SamplingParams(None, None, table)


def sample_params_tensor(table, device):
    """SAMPLE_PARAMS_DTYPE [B] (host) -> int32 [B, 3] on the device: the bytes of t2h_sample_params[B]"""
    assert table.dtype == SAMPLE_PARAMS_DTYPE and table.ndim == 1
    return torch.from_numpy(np.ascontiguousarray(table).view(np.int32).reshape(-1, 3).copy()).to(device)


def _chk_params(params, rows_per_sample, n):
    """a device table for the *_per_sample entry points: int32 [B, 3] with B * rows_per_sample == n"""
    T = int(rows_per_sample)
    assert params.dtype == torch.int32 and params.is_cuda and params.is_contiguous() and params.dim() == 2
    assert params.shape[1] == 3 and T > 0 and params.shape[0] * T == n, (tuple(params.shape), T, n)
    return T


def truncation_threshold_per_row(logits, params, rows_per_sample, scope=0):
    """truncation_threshold with row r's rules taken from params[r // rows_per_sample] (sample_params_tensor;
    t2h_truncation_threshold_per_row) -> theta f32 [n_rows], kept int32 [n_rows]"""
    _chk_f32(logits)
    assert logits.dim() == 2 and logits.is_contiguous()
    n_rows, n_class = logits.shape
    T = _chk_params(params, rows_per_sample, n_rows)
    theta = torch.empty(n_rows, dtype=torch.float32, device=logits.device)
    kept = torch.empty(n_rows, dtype=torch.int32, device=logits.device)
    check(_lib.load().t2h_truncation_threshold_per_row(_p(logits), n_rows, n_class, _p(params), T, int(scope), _p(theta),
                                                       _p(kept), _stream()), 't2h_truncation_threshold_per_row')
    return theta, kept


def truncation_threshold(logits, top_k=None, top_p=None, scope=0):
    """The row thresholds of truncated sampling by themselves (t2h_truncation_threshold): logits f32 [n_rows, n_class]
    (already divided by the temperature) -> theta f32 [n_rows], kept int32 [n_rows].  scope 0 / 1: the workgroup /
    wave form of the selection, as sample_heads / confidence_tail run it."""
    _chk_f32(logits)
    assert logits.dim() == 2 and logits.is_contiguous()
    n_rows, n_class = logits.shape
    k, p_q = truncation_settings(top_k, top_p, n_class)
    theta = torch.empty(n_rows, dtype=torch.float32, device=logits.device)
    kept = torch.empty(n_rows, dtype=torch.int32, device=logits.device)
    check(_lib.load().t2h_truncation_threshold(_p(logits), n_rows, n_class, k, p_q, int(scope), _p(theta), _p(kept),
                                               _stream()), 't2h_truncation_threshold')
    return theta, kept


def _philox_fields(a, numel, device, **fields):
    """philox_seed (philox_offset: of a whole-tensor draw of `numel` floats): ints, or int64 device tensors a replay reads"""
    for name, v in fields.items():
        if torch.is_tensor(v):
            assert v.dtype == torch.int64 and v.is_cuda and (v.numel() == 1 if name == 'philox_seed' else v.numel() >= 1)
            setattr(a, name + '_dev', v.data_ptr())
        else:
            setattr(a, name, int(v) & 0xFFFFFFFFFFFFFFFF)
    a.philox_grid_threads = torch_draw_geometry(numel, device)[0]


def sample_heads(hidden, lnf_g, lnf_b, w_heads, expo_by_head, rows, n_rows, tex, temp, x_t, out_idx, split=True,
                 philox=None, hidden_compact=False, row_noise=None, logits_ws=None, top_k=0, top_p=1.0, params=None,
                 rows_per_sample=None, logp=None, targets=None, rank=None, seed_img=None, img_rows=None):
    """All heads in one launch: `rows` (int32, first n_rows valid) are the changed token
    rows, expo_by_head {head: [n, n_class] Exp(1) draw}, w_heads [n_heads, n_class, C],
    out_idx [n_heads, n].  philox = (seed, {head: generator offset}): the noise of the listed heads is
    computed in the kernel as the corresponding elements of torch's full-tensor exponential_ draws
    instead of being read from expo_by_head.  row_noise (row lists that mix sampling steps):
    ('philox', seed, offsets int64 [>= n_rows][, rng_rows int32 [>= n_rows]]) = per-listed-row generator offsets (and
    the rows of the reference's draw they belong to, if the samples were reordered), or
    ('explicit', expo_rows f32 [*, n_class], slots int32 [>= n_rows]) = per-listed-row explicit draws.
    top_k / top_p: truncated sampling (truncation_settings; the defaults are off = the kernels without it).
    params (sample_params_tensor) + rows_per_sample: per-image controls (t2h_sample_heads_per_sample) -- row r is drawn
    with params[r // rows_per_sample]; temp / top_k / top_p are then not read.
    logp (f32, >= n elements, indexed by token row like x_t; None = off, the kernels without it): every listed row
    also gets the log-probability of its token under the full softmax of logits / temp.
    targets (int64 [n_heads, n], the layout of out_idx; None = off): scoring (t2h_score_heads[_per_sample], DESIGN.md
    4.6g) -- the token of a listed row is read from targets[tex[row]][row] instead of drawn, no noise is read, logp is
    required; rank (int32, >= n elements, optional): the number of classes with a strictly greater logit.
    seed_img (int64 [n / img_rows] on the device, seeds_tensor) + img_rows: per-image seeds -- with a
    'philox' row_noise, listed row r is drawn with seed seed_img[r // img_rows] on row r % img_rows of its own image's
    [img_rows, n_class] draw (row_noise's seed is not read; its rng_rows, if any, still name the noise row)."""
    _chk_f32(hidden, lnf_g, lnf_b, w_heads, *expo_by_head.values())
    score = None
    if targets is not None:
        _chk_i64(targets)
        assert logp is not None and targets.is_contiguous() and tuple(targets.shape) == tuple(out_idx.shape)
        score = _lib.ScoreOut()
        score.targets = targets.data_ptr()
        if rank is not None:
            assert rank.dtype == torch.int32 and rank.is_cuda and rank.is_contiguous() and rank.numel() >= out_idx.shape[1]
            score.rank = rank.data_ptr()
    else:
        assert rank is None
    if logp is not None:
        _chk_f32(logp)
        assert logp.is_contiguous() and logp.numel() >= out_idx.shape[1], (tuple(logp.shape), tuple(out_idx.shape))
    trunc = truncation_settings(top_k, top_p, w_heads.shape[1]) if params is None else (0, 0)
    if int(n_rows) == 0:
        return
    C = hidden.shape[1]
    n = out_idx.shape[1]
    assert hidden.shape[0] == (int(n_rows) if hidden_compact else n)
    n_heads, n_class = w_heads.shape[0], w_heads.shape[1]
    assert w_heads.is_contiguous() and out_idx.is_contiguous() and out_idx.shape == (n_heads, n)
    a = _lib.SampleHeadsArgs()
    a.hidden, a.lnf_gamma, a.lnf_beta, a.w_heads = (hidden.data_ptr(), lnf_g.data_ptr(), lnf_b.data_ptr(),
                                                    w_heads.data_ptr())
    for h, e in expo_by_head.items():
        assert e.shape == (n, n_class) and e.is_contiguous()
        a.expo[h] = e.data_ptr()
    a.rows, a.tex, a.x_t, a.out_idx = rows.data_ptr(), tex.data_ptr(), x_t.data_ptr(), out_idx.data_ptr()
    a.temp, a.n_rows, a.n, a.C, a.n_class, a.n_heads = (float(temp) if params is None else 1.0), int(n_rows), n, C, n_class, n_heads
    a.hidden_compact = int(bool(hidden_compact))
    a.top_k, a.top_p_q = trunc
    if logp is not None:
        a.logp = logp.data_ptr()
    if (split or philox is not None or hidden_compact or row_noise is not None or score is not None) and n_rows > 0:
        # logits scratch: 8 workgroups per row share the weight stream
        ws = logits_ws if logits_ws is not None else torch.empty((int(n_rows), n_class), device=hidden.device,
                                                                 dtype=torch.float32)
        assert ws.numel() >= int(n_rows) * n_class and ws.dtype == torch.float32
        a.logits_ws = ws.data_ptr()
    if row_noise is not None:
        if row_noise[0] == 'philox':
            _, seed, offs = row_noise[:3]
            assert offs.dtype == torch.int64 and offs.is_cuda and offs.numel() >= int(n_rows)
            a.row_philox_offset = offs.data_ptr()
            if len(row_noise) > 3 and row_noise[3] is not None:  # rows of the reference's draw (reordered samples)
                rr = row_noise[3]
                assert rr.dtype == torch.int32 and rr.is_cuda and rr.numel() >= int(n_rows)
                a.rng_rows = rr.data_ptr()
            if seed_img is not None:
                T_img = int(img_rows)
                assert seed_img.dtype == torch.int64 and seed_img.is_cuda and seed_img.is_contiguous()
                assert T_img > 0 and seed_img.numel() * T_img == n, (seed_img.numel(), T_img, n)
                a.philox_seed_img, a.img_rows = seed_img.data_ptr(), T_img
                a.philox_grid_threads = torch_draw_geometry(T_img * n_class, hidden.device)[0]  # ONE image's draw
            else:
                _philox_fields(a, n * n_class, hidden.device, philox_seed=seed)  # (a tensor: the seed of a replayed round)
        else:
            assert seed_img is None, 'per-image seeds draw in the kernel: no explicit noise'
            _, erows, slots = row_noise
            _chk_f32(erows)
            assert erows.is_contiguous() and erows.shape[-1] == n_class
            assert slots.dtype == torch.int32 and slots.is_cuda and slots.numel() >= int(n_rows)
            a.expo_rows, a.expo_slot = erows.data_ptr(), slots.data_ptr()
    elif philox is not None:
        assert seed_img is None
        _philox_fields(a, n * n_class, hidden.device, philox_seed=philox[0])
        for h, off in philox[1].items():
            a.philox_offset[h] = int(off)
    if score is not None:
        if params is not None:
            T = _chk_params(params, rows_per_sample, n)
            return check(_lib.load().t2h_score_heads_per_sample(ctypes.byref(a), ctypes.byref(score), _p(params), T,
                                                                _stream()), 't2h_score_heads_per_sample')
        return check(_lib.load().t2h_score_heads(ctypes.byref(a), ctypes.byref(score), _stream()), 't2h_score_heads')
    if params is not None:
        T = _chk_params(params, rows_per_sample, n)
        return check(_lib.load().t2h_sample_heads_per_sample(ctypes.byref(a), _p(params), T, _stream()),
                     't2h_sample_heads_per_sample')
    check(_lib.load().t2h_sample_heads(ctypes.byref(a), _stream()), 't2h_sample_heads')


def confidence_group_ws(n, n_heads, device):
    """Workspace of confidence_tail's grouping launch (int32)."""
    return torch.empty(int(_lib.load().t2h_confidence_group_ws_ints(int(n), int(n_heads))), dtype=torch.int32,
                       device=device)


def confidence_tail(hidden, lnf_g, lnf_b, w_heads, tex, x_t, mask_id, temp, noise, tok, conf, group_ws=None,
                    logits_ws=None, top_k=0, top_p=1.0, params=None, rows_per_sample=None):
    """Token and confidence of EVERY masked row (t2h_confidence_tail): hidden f32 [n, C], w_heads [n_heads, n_class, C],
    tex / x_t int64 [n] -> tok int32 [n] (-1 where not masked), conf f32 [n] (-inf where not masked).  noise:
    ('explicit', E f32 [n, n_class]) or ('philox', seed, offset) = the elements of torch's
    `empty(n, n_class).exponential_()` at that generator state.  top_k / top_p: truncated sampling
    (truncation_settings) -- changes tok only, conf stays the log-probability under the full softmax.  params +
    rows_per_sample: per-image controls as in sample_heads (t2h_confidence_tail_per_sample)."""
    _chk_f32(hidden, lnf_g, lnf_b, w_heads, conf)
    _chk_i64(tex, x_t)
    n, C = hidden.shape
    n_heads, n_class = w_heads.shape[0], w_heads.shape[1]
    assert hidden.is_contiguous() and w_heads.is_contiguous() and tex.numel() == n and x_t.numel() == n
    assert tok.dtype == torch.int32 and tok.is_cuda and tok.numel() == n and conf.numel() == n
    dev = hidden.device
    group_ws = group_ws if group_ws is not None else confidence_group_ws(n, n_heads, dev)
    logits_ws = logits_ws if logits_ws is not None else torch.empty((n, n_class), dtype=torch.float32, device=dev)
    assert group_ws.dtype == torch.int32 and logits_ws.dtype == torch.float32 and logits_ws.numel() >= n * n_class
    assert group_ws.numel() >= int(_lib.load().t2h_confidence_group_ws_ints(n, n_heads))
    a = _lib.ConfidenceTailArgs()
    a.hidden, a.lnf_gamma, a.lnf_beta, a.w_heads = hidden.data_ptr(), lnf_g.data_ptr(), lnf_b.data_ptr(), w_heads.data_ptr()
    a.tex, a.x_t, a.mask_id, a.temp = tex.data_ptr(), x_t.data_ptr(), int(mask_id), (float(temp) if params is None else 1.0)
    a.n, a.C, a.n_class, a.n_heads = n, C, n_class, n_heads
    a.top_k, a.top_p_q = truncation_settings(top_k, top_p, n_class) if params is None else (0, 0)
    if noise[0] == 'explicit':
        e = noise[1]
        _chk_f32(e)
        assert e.is_contiguous() and e.numel() == n * n_class
        a.expo = e.data_ptr()
    else:
        _philox_fields(a, n * n_class, dev, philox_seed=noise[1], philox_offset=noise[2])
    a.group_ws, a.logits_ws, a.tok, a.conf = group_ws.data_ptr(), logits_ws.data_ptr(), tok.data_ptr(), conf.data_ptr()
    if params is not None:
        T = _chk_params(params, rows_per_sample, n)
        check(_lib.load().t2h_confidence_tail_per_sample(ctypes.byref(a), _p(params), T, _stream()),
              't2h_confidence_tail_per_sample')
        return tok, conf
    check(_lib.load().t2h_confidence_tail(ctypes.byref(a), _stream()), 't2h_confidence_tail')
    return tok, conf


def confidence_commit(conf, tok, tex, noise, k, tau, mask_id, x_t, out, n_class, scores=None, per_sample=False,
                      logp=None):
    """Commits, per sample, the k[b] masked rows with the largest score conf + tau * gumbel(U) (t2h_confidence_commit):
    x_t int64 [B, T] and out int64 [n_heads, B * T] are updated in place.  k int32 [>= B] and tau f32 [>= 1] are device
    tensors; noise: ('explicit', U f32 [B * T]) or ('philox', seed, offset) = the elements of torch's `rand(B * T)`.
    per_sample: tau is f32 [>= B], sample b scores with tau[b] (t2h_confidence_commit_per_sample).
    logp (f32, >= B * T elements; None = off): a committed row gets logp[row] = conf[row], other rows are not written."""
    _chk_f32(conf, tau)
    _chk_i64(tex, x_t, out)
    B, T = x_t.shape
    n = B * T
    n_heads = out.shape[0]
    assert tuple(out.shape) == (n_heads, n) and conf.numel() == n and tok.numel() == n and tex.numel() == n
    assert tok.dtype == torch.int32 and k.dtype == torch.int32 and k.is_cuda and k.numel() >= B
    assert tau.numel() >= (B if per_sample else 1)
    a = _lib.ConfidenceCommitArgs()
    a.conf, a.tok, a.tex = conf.data_ptr(), tok.data_ptr(), tex.data_ptr()
    if noise[0] == 'explicit':
        u = noise[1]
        _chk_f32(u)
        assert u.is_contiguous() and u.numel() == n
        a.u = u.data_ptr()
    else:
        _philox_fields(a, n, x_t.device, philox_seed=noise[1], philox_offset=noise[2])
    a.k, a.tau, a.mask_id, a.x_t, a.out = k.data_ptr(), tau.data_ptr(), int(mask_id), x_t.data_ptr(), out.data_ptr()
    if scores is not None:
        _chk_f32(scores)
        assert scores.numel() == n
        a.scores = scores.data_ptr()
    a.B, a.T, a.n_heads, a.n_class = B, T, n_heads, int(n_class)
    if logp is not None:
        _chk_f32(logp)
        assert logp.is_contiguous() and logp.numel() >= n
        a.logp = logp.data_ptr()
    if per_sample:
        return check(_lib.load().t2h_confidence_commit_per_sample(ctypes.byref(a), _stream()),
                     't2h_confidence_commit_per_sample')
    check(_lib.load().t2h_confidence_commit(ctypes.byref(a), _stream()), 't2h_confidence_commit')


def logp_summary(logp, B=None, T=None):
    """Per-image summary of per-token log-probabilities (t2h_logp_summary): logp f32 [B, T] (or flat with B, T given),
    NaN = never drawn -> (sum f32 [B], count int32 [B], min f32 [B]); an image's numbers do not depend on its place in
    the batch.  An image without a drawn row: (0, 0, +inf)."""
    _chk_f32(logp)
    if B is None:
        B, T = logp.shape
    assert logp.is_contiguous() and logp.numel() == int(B) * int(T)
    dev = logp.device
    s, m = torch.empty(int(B), dtype=torch.float32, device=dev), torch.empty(int(B), dtype=torch.float32, device=dev)
    c = torch.empty(int(B), dtype=torch.int32, device=dev)
    check(_lib.load().t2h_logp_summary(_p(logp), int(B), int(T), _p(s), _p(c), _p(m), _stream()), 't2h_logp_summary')
    return s, c, m


def sample_head(hidden, lnf_g, lnf_b, w_head, expo, changes, tex, head, temp, x_t, out_idx):
    _chk_f32(hidden, lnf_g, lnf_b, w_head, expo)
    n, C = hidden.shape
    n_class = w_head.shape[0]
    assert expo.shape == (n, n_class) and expo.is_contiguous() and w_head.is_contiguous()
    check(_lib.load().t2h_sample_head(_p(hidden), _p(lnf_g), _p(lnf_b), _p(w_head), _p(expo),
                                      _p(changes), _p(tex), int(head), float(temp), _p(x_t),
                                      _p(out_idx), n, C, n_class, _stream()), 't2h_sample_head')


def q_sample(x0, u, t, num_timesteps, mask_id):
    """x0 int64 [B, T], u f32 [B, T] uniform draw, t int64 [B] -> (x_t int64 [B, T], mask uint8 [B, T])."""
    _chk_i64(x0, t)
    _chk_f32(u)
    B, T = x0.shape
    x_t = torch.empty_like(x0)
    mask = torch.empty((B, T), dtype=torch.uint8, device=x0.device)
    check(_lib.load().t2h_q_sample(_p(x0.contiguous()), _p(u.contiguous()), _p(t.contiguous()), int(num_timesteps),
                                   int(mask_id), _p(x_t), _p(mask), B, T, _stream()), 't2h_q_sample')
    return x_t, mask


def masked_ce_heads(hidden, lnf_g, lnf_b, w_heads, tex, mask, gt_lists, B, T):
    """-> (ce_rows f32 [B*T], ce_samples f32 [B]): summed 18-head cross entropy of the masked tokens."""
    _chk_f32(hidden, lnf_g, lnf_b, w_heads)
    _chk_i64(tex, gt_lists)
    n, C = hidden.shape
    n_heads, n_class = w_heads.shape[0], w_heads.shape[1]
    assert n == B * T and gt_lists.shape == (n_heads, n) and gt_lists.is_contiguous() and w_heads.is_contiguous()
    ce_rows = torch.empty(n, dtype=torch.float32, device=hidden.device)
    ce_samples = torch.empty(B, dtype=torch.float32, device=hidden.device)
    check(_lib.load().t2h_masked_ce_heads(_p(hidden), _p(lnf_g), _p(lnf_b), _p(w_heads), _p(tex), _p(mask),
                                          _p(gt_lists), _p(ce_rows), _p(ce_samples), B, T, C, n_class, n_heads,
                                          _stream()), 't2h_masked_ce_heads')
    return ce_rows, ce_samples


def vq_l2_argmin(z, codebook):
    _chk_f32(z, codebook)
    assert z.is_contiguous() and codebook.is_contiguous()
    n, d = z.shape
    idx = torch.empty((n, ), device=z.device, dtype=torch.int64)
    check(_lib.load().t2h_vq_l2_argmin_f32(_p(z), _p(codebook), _p(idx), n, codebook.shape[0], d,
                                           _stream()), 't2h_vq_l2_argmin_f32')
    return idx


def vq_argmin_tex(z, books, tex, fold_hw=None):
    """Texture-routed codebook argmin (encode side).  z: latent rows [n, d], or with
    fold_hw=(h, w) the NHWC map rows [B*2h*2w, d/4] whose 2x2 patches are quantised;
    books [n_books, n_e, d]; tex int64 [n].  Returns idx_lists int64 [n_books, n] (-1
    where the row is not of that texture)."""
    _chk_f32(z, books)
    _chk_i64(tex)
    nb, n_e, d = books.shape
    n = tex.numel()
    fh, fw = fold_hw or (0, 0)
    assert z.is_contiguous() and books.is_contiguous()
    assert z.numel() == n * d, (tuple(z.shape), n, d)
    out = torch.empty((nb, n), device=z.device, dtype=torch.int64)
    check(_lib.load().t2h_vq_argmin_tex_f32(_p(z), _p(books), _p(tex), _p(out), n, nb, n_e, d, fh, fw,
                                            _stream()), 't2h_vq_argmin_tex_f32')
    return out


def vq_fit_books(z, books, want_index=True):
    """All-codebook fit.  z: latent rows [n, 256]; books [n_books, n_e, 256].  Returns
    (dmin f32 [n, n_books], jmin i32 [n, n_books] or None): per row and book the least expanded distance and the
    first code that attains it (+inf / -1 where no code gives a comparable distance)."""
    _chk_f32(z, books)
    nb, n_e, d = books.shape
    assert z.dim() == 2 and z.shape[1] == d, (tuple(z.shape), d)
    assert z.is_contiguous() and books.is_contiguous()
    n = z.shape[0]
    dmin = torch.empty((n, nb), device=z.device, dtype=torch.float32)
    jmin = torch.empty((n, nb), device=z.device, dtype=torch.int32) if want_index else None
    check(_lib.load().t2h_vq_fit_books_f32(_p(z), _p(books), _p(dmin), _p(jmin), n, nb, n_e, d, _stream()),
          't2h_vq_fit_books_f32')
    return dmin, jmin


def vq_fit_force_tile(rows):
    """Row tile of vq_fit_books for the calling thread (32 / 64 / 128; 0 = automatic).  Returns the old value."""
    return _lib.load().t2h_vq_fit_force_tile(int(rows))


def texture_vote(dmin, segm_tok, B):
    """Region vote over a fit.  dmin f32 [B*T, n_books]; segm_tok i64 [B, T] (or [B*T]) parsing
    labels of the token cells.  Returns (cost f64 [B, 3, n_books], count i32 [B, 3], attr i64 [B, 3]); the groups
    are upper, lower, outer."""
    _chk_f32(dmin)
    _chk_i64(segm_tok)
    assert dmin.dim() == 2 and dmin.is_contiguous()
    n, nb = dmin.shape
    assert B > 0 and n % B == 0 and segm_tok.numel() == n, (B, n, segm_tok.numel())
    cost = torch.empty((B, 3, nb), device=dmin.device, dtype=torch.float64)
    count = torch.empty((B, 3), device=dmin.device, dtype=torch.int32)
    attr = torch.empty((B, 3), device=dmin.device, dtype=torch.int64)
    check(_lib.load().t2h_texture_vote(_p(dmin), _p(segm_tok), B, n // B, nb, _p(cost), _p(count), _p(attr),
                                       _stream()), 't2h_texture_vote')
    return cost, count, attr


def codebook_gather_tex(idx_lists, tex, books):
    """idx_lists [18, n] i64, tex [n] i64, books [18, n_e, e_dim] -> [n, e_dim]."""
    _chk_i64(idx_lists, tex)
    _chk_f32(books)
    nb, n_e, e_dim = books.shape
    n = tex.numel()
    out = torch.empty((n, e_dim), device=books.device, dtype=torch.float32)
    check(_lib.load().t2h_codebook_gather_tex_f32(_p(idx_lists), _p(tex), _p(books), _p(out), n, nb,
                                                  n_e, e_dim, _stream()),
          't2h_codebook_gather_tex_f32')
    return out


def codebook_gather_fold(idx_lists, tex, books, B, h, w):
    """books [18, n_e, C*4] -> NHWC rows [B*2h*2w, C]."""
    _chk_i64(idx_lists, tex)
    _chk_f32(books)
    nb, n_e, e4 = books.shape
    C = e4 // 4
    out = torch.empty((B * 2 * h * 2 * w, C), device=books.device, dtype=torch.float32)
    check(_lib.load().t2h_codebook_gather_fold_f32(_p(idx_lists), _p(tex), _p(books), _p(out), B, h, w,
                                                   nb, n_e, C, _stream()),
          't2h_codebook_gather_fold_f32')
    return out


def routed_head_argmax(feat, w, b, tex, n_heads, cf, n_class):
    """feat [n, n_heads*cf]; w [n_heads, n_class, cf]; b [n_heads, n_class]
    -> out_lists [n_heads, n] i64 (-1 off-texture)."""
    _chk_f32(feat, w, b)
    _chk_i64(tex)
    n = feat.shape[0]
    out = torch.empty((n_heads, n), device=feat.device, dtype=torch.int64)
    check(_lib.load().t2h_routed_head_argmax(_p(feat), _rows(feat), _p(w), _p(b), _p(tex), _p(out), n,
                                             n_heads, cf, n_class, _stream()),
          't2h_routed_head_argmax')
    return out


def routed_head_sample(feat, w, b, tex, n_heads, cf, n_class, temp=1.0, top_k=None, top_p=None, params=None,
                       rows_per_sample=None, expo=None, philox=None, noise_rows=None, noise_row0=0, want_logp=False,
                       want_logits=False):
    """routed_head_argmax with a draw in place of the maximum (t2h_routed_head_sample): the detail code
    of row r is drawn from softmax(head(feat[r]) / temp), truncated by top_k / top_p (truncation_settings; None = off).
    params (sample_params_tensor) + rows_per_sample: row r uses params[r // rows_per_sample]; temp / top_k / top_p are
    then not read.  Noise: expo f32 [n, n_class], or philox = (seed, offset) of torch's generator before a
    `torch.empty(noise_rows, n_class).exponential_()` draw (noise_rows defaults to n), of which this launch takes rows
    noise_row0 .. noise_row0 + n - 1.  -> out_lists [n_heads, n] i64 (-1 off-texture); with want_logp / want_logits
    the tuple (out_lists, logp f32 [n] or None, logits f32 [n, n_class] or None)."""
    _chk_f32(feat, w, b)
    _chk_i64(tex)
    n = feat.shape[0]
    assert w.is_contiguous() and b.is_contiguous() and tex.is_contiguous() and tex.numel() == n
    assert tuple(w.shape) == (n_heads, n_class, cf) and b.numel() == n_heads * n_class
    if (expo is None) == (philox is None):
        raise ValueError('routed_head_sample: give exactly one of expo (an explicit draw) or philox (seed, offset)')
    a = _lib.RoutedSampleArgs()
    if params is None:
        if isinstance(temp, bool) or not isinstance(temp, numbers.Real) or not float(temp) > 0.0 or float(temp) == float('inf'):
            raise ValueError(f'temp must be a finite number > 0, got {temp!r}')
        a.temp = float(temp)
        a.top_k, a.top_p_q = truncation_settings(top_k, top_p, n_class)
    out = torch.empty((n_heads, n), device=feat.device, dtype=torch.int64)
    logp = torch.empty(n, device=feat.device, dtype=torch.float32) if want_logp else None
    logits = torch.empty((n, n_class), device=feat.device, dtype=torch.float32) if want_logits else None
    a.feat, a.ldf, a.w, a.b, a.tex, a.out_lists = feat.data_ptr(), _rows(feat), w.data_ptr(), b.data_ptr(), tex.data_ptr(), out.data_ptr()
    a.n, a.n_heads, a.Cf, a.n_class = n, int(n_heads), int(cf), int(n_class)
    if expo is not None:
        _chk_f32(expo)
        assert expo.is_contiguous() and tuple(expo.shape) == (n, n_class)
        a.expo = expo.data_ptr()
    else:
        total = n if noise_rows is None else int(noise_rows)
        assert 0 <= int(noise_row0) and int(noise_row0) + n <= total
        a.philox_seed, a.philox_offset = int(philox[0]) & 0xFFFFFFFFFFFFFFFF, int(philox[1])
        a.philox_grid_threads = torch_draw_geometry(total * n_class, feat.device)[0]
        a.noise_row0 = int(noise_row0)
    a.logp = logp.data_ptr() if logp is not None else None
    a.logits_ws = logits.data_ptr() if logits is not None else None
    T = 0
    if params is not None:
        T = _chk_params(params, rows_per_sample, n)
    check(_lib.load().t2h_routed_head_sample(ctypes.byref(a), _p(params), T, _stream()), 't2h_routed_head_sample')
    return (out, logp, logits) if (want_logp or want_logits) else out


def onehot_nhwc(segm, n_cls, cpad):
    _chk_f32(segm)
    n_pix = segm.numel()
    out = torch.empty((n_pix, cpad), device=segm.device, dtype=torch.float32)
    check(_lib.load().t2h_onehot_nhwc_f32(_p(segm.contiguous()), _p(out), n_pix, n_cls, cpad, _stream()),
          't2h_onehot_nhwc_f32')
    return out


def nchw_to_nhwc(x, cpad=None):
    """x [B,C,H,W] -> rows [B*H*W, cpad or C] (extra channels zero)."""
    _chk_f32(x)
    B, C, H, W = x.shape
    ld = cpad or C
    out = (torch.zeros if ld != C else torch.empty)((B * H * W, ld), device=x.device,
                                                   dtype=torch.float32)
    check(_lib.load().t2h_nchw_to_nhwc_f32(_p(x.contiguous()), _p(out), B, C, H * W, ld, _stream()),
          't2h_nchw_to_nhwc_f32')
    return out


def nhwc_to_nchw(x, B, H, W, C=None):
    _chk_f32(x)
    C = C or x.shape[1]
    out = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32)
    check(_lib.load().t2h_nhwc_to_nchw_f32(_p(x), _rows(x), _p(out), B, C, H * W, _stream()),
          't2h_nhwc_to_nchw_f32')
    return out


def maxpool2(x, B, H, W):
    _chk_f32(x)
    C = x.shape[1]
    out = torch.empty((B * (H // 2) * (W // 2), C), device=x.device, dtype=torch.float32)
    check(_lib.load().t2h_maxpool2_nhwc_f32(_p(x), _rows(x), _p(out), B, H, W, C, _stream()),
          't2h_maxpool2_nhwc_f32')
    return out


def bilinear_up2(x, B, H, W):
    _chk_f32(x)
    assert x.is_contiguous()
    C = x.shape[1]
    out = torch.empty((B * 4 * H * W, C), device=x.device, dtype=torch.float32)
    check(_lib.load().t2h_bilinear_up2_nhwc_f32(_p(x), _p(out), B, H, W, C, _stream()),
          't2h_bilinear_up2_nhwc_f32')
    return out


def argmax_rows(x, n=None):
    _chk_f32(x)
    rows = x.shape[0]
    n = n or x.shape[1]
    out = torch.empty((rows, ), device=x.device, dtype=torch.int64)
    check(_lib.load().t2h_argmax_rows_f32(_p(x), _rows(x), _p(out), rows, n, _stream()),
          't2h_argmax_rows_f32')
    return out


def image_epilogue(dec, B, H, W, want_u8=False):
    """dec rows [B*H*W, >=3] -> (img f32 [B,3,H,W] in [0,1], u8 [B,H,W,3] or None)."""
    _chk_f32(dec)
    img = torch.empty((B, 3, H, W), device=dec.device, dtype=torch.float32)
    u8 = torch.empty((B, H, W, 3), device=dec.device, dtype=torch.uint8) if want_u8 else None
    check(_lib.load().t2h_image_epilogue(_p(dec), _rows(dec), _p(img), _p(u8), B, H * W, _stream()),
          't2h_image_epilogue')
    return img, u8


COMPOSITE_R_MAX = 32  # widest blur radius of t2h_composite_region_f32 (taps [2R + 1])
_composite_taps = {}


def composite_taps_host(r_lo):
    """The blur of ops.composite_region -> float32 numpy [2R + 1]: a Gaussian of sigma = r_lo / 4 cut at
    R = min(32, ceil(3 sigma)), computed and normalised to sum 1 in float64, then rounded to fp32."""
    sigma = int(r_lo) / 4.0
    R = min(COMPOSITE_R_MAX, int(np.ceil(3.0 * sigma)))
    k = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-0.5 * (k / sigma) ** 2)
    return (g / g.sum()).astype(np.float32)


def _check_composite_radii(r_hi, r_lo, names=('r_hi', 'r_lo')):
    for name, v in zip(names, (r_hi, r_lo)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f'compositing: {name} must be an integer number of pixels, got {v!r}')
    if not 1 <= r_hi <= r_lo <= 64:
        raise ValueError(f'compositing: need 1 <= {names[0]} <= {names[1]} <= 64, got {names[0]}={r_hi}, '
                         f'{names[1]}={r_lo}')


def composite_region(dec, photo, keep, cells, r_hi=4, r_lo=32, photo_signed=True, want_u8=False):
    """Two-band compositing of an edited region into its source photo (t2h_composite_region_f32).
    dec f32 [B, 3, H, W] in [0, 1] (image_epilogue's image), photo f32 [B, 3, H, W] (photo_signed: in [-1, 1], read as
    ((x + 1) / 2).clamp(0, 1)), keep uint8 [B, th * tw] (region_keep: 0 = edited cell), cells = (th, tw).  With d the
    Chebyshev distance of a pixel to the nearest edited cell: the decoder's pixels where d == 0, the photo's where
    d >= r_lo, in between the photo plus the decoder's blurred offset fading over r_lo pixels and its detail over r_hi.
    -> (img f32 [B, 3, H, W], u8 [B, H, W, 3] or None).  No host synchronisation, the generator is not touched."""
    _chk_f32(dec, photo)
    _check_composite_radii(r_hi, r_lo)
    if dec.dim() != 4 or dec.shape[1] != 3 or not dec.is_contiguous():
        raise ValueError(f'composite_region: dec must be a contiguous [B, 3, H, W] image, got {tuple(dec.shape)}')
    if tuple(photo.shape) != tuple(dec.shape) or not photo.is_contiguous():
        raise ValueError(f'composite_region: photo must be contiguous and shaped like dec {tuple(dec.shape)}, got '
                         f'{tuple(photo.shape)}')
    B, _, H, W = dec.shape
    th, tw = cells
    if tuple(keep.shape) != (B, th * tw):
        raise ValueError(f'composite_region: keep must be [{B}, {th * tw}], got {tuple(keep.shape)}')
    _chk_u8(keep, B * th * tw)
    key = (int(r_lo), dec.device)
    taps = _composite_taps.get(key)
    if taps is None:  # (built once per r_lo and device, outside any capture)
        taps = _composite_taps[key] = torch.from_numpy(composite_taps_host(r_lo)).to(dec.device)
    img = torch.empty_like(dec)
    u8 = torch.empty((B, H, W, 3), device=dec.device, dtype=torch.uint8) if want_u8 else None
    check(_lib.load().t2h_composite_region_f32(_p(dec), _p(photo), _p(keep), _p(taps), _p(img), _p(u8), B, H, W, th, tw,
                                               int(r_hi), int(r_lo), (taps.numel() - 1) // 2, int(bool(photo_signed)),
                                               _stream()), 't2h_composite_region_f32')
    return img, u8


RECOLOR_GROUPS = {'upper': (1, 4), 'lower': (3, 5, 21), 'outer': (2, )}  # the classes of t2h_texture_map
RECOLOR_G_MAX, RECOLOR_FEATHER_MAX, RECOLOR_GAIN_MAX = 4, 8, 16.0
RECOLOR_STRIPE = 16  # image rows per partial row of t2h_region_color_stats (its workspace: [B, ceil(H / 16), G, 8] f64)


def recolor_group_bits(groups):
    """groups of region_color_stats / recolor_region: 1 .. 4 entries, each a name of RECOLOR_GROUPS or an iterable of
    parsing label ids in [0, 64), pairwise disjoint -> list of label bit sets (ValueError otherwise)."""
    if isinstance(groups, (str, bytes)) or not hasattr(groups, '__len__') or not 1 <= len(groups) <= RECOLOR_G_MAX:
        raise ValueError(f'recolor: groups must be a list of 1 .. {RECOLOR_G_MAX} group names or label lists, got {groups!r}')
    out = []
    for grp in groups:
        if isinstance(grp, str):
            if grp not in RECOLOR_GROUPS:
                raise ValueError(f'recolor: unknown group {grp!r} (names: {sorted(RECOLOR_GROUPS)}; or give label ids)')
            grp = RECOLOR_GROUPS[grp]
        try:
            labels = list(grp)
        except TypeError:
            raise ValueError(f'recolor: a group is a name or a list of label ids, got {grp!r}') from None
        bits = 0
        for lb in labels:
            if isinstance(lb, bool) or not isinstance(lb, numbers.Integral) or not 0 <= int(lb) < 64:
                raise ValueError(f'recolor: label ids must be integers in [0, 64), got {lb!r}')
            bits |= 1 << int(lb)
        if bits == 0:
            raise ValueError('recolor: a group needs at least one label id')
        if any(bits & b for b in out):
            raise ValueError(f'recolor: the groups must be disjoint, {labels} shares a label with an earlier group')
        out.append(bits)
    return out


def _check_recolor_params(luma, gain_max, feather):
    if isinstance(feather, bool) or not isinstance(feather, numbers.Integral) or not 0 <= feather <= RECOLOR_FEATHER_MAX:
        raise ValueError(f'recolor: feather must be an integer number of pixels in [0, {RECOLOR_FEATHER_MAX}], got {feather!r}')
    if isinstance(luma, bool) or not isinstance(luma, numbers.Real) or not 0.0 <= float(luma) <= 1.0:
        raise ValueError(f'recolor: luma must lie in [0, 1], got {luma!r}')
    if isinstance(gain_max, bool) or not isinstance(gain_max, numbers.Real) or not 1.0 <= float(gain_max) <= RECOLOR_GAIN_MAX:
        raise ValueError(f'recolor: gain_max must lie in [1, {RECOLOR_GAIN_MAX:g}], got {gain_max!r}')


def _recolor_inputs(name, img, segm):
    _chk_f32(img, segm)
    if img.dim() != 4 or img.shape[1] != 3 or not img.is_contiguous():
        raise ValueError(f'{name}: img must be a contiguous [B, 3, H, W] image, got {tuple(img.shape)}')
    B, _, H, W = img.shape
    if tuple(segm.shape) not in ((B, H, W), (B, 1, H, W)) or not segm.is_contiguous():
        raise ValueError(f'{name}: segm must be a contiguous [{B}, {H}, {W}] (or [{B}, 1, {H}, {W}]) parsing map, got '
                         f'{tuple(segm.shape)}')
    return B, H, W


def region_color_stats(img, segm, groups, img_signed=False):
    """Colour statistics of parsing-map regions (t2h_region_color_stats).  img f32 [B, 3, H, W]
    (img_signed: in [-1, 1], read as ((x + 1) / 2).clamp(0, 1)), segm f32 [B, H, W] or [B, 1, H, W] (the parsing map as
    the tokenizer reads it), groups: see recolor_group_bits.  -> f64 [B, G, 8] on the device =
    {n, mY, mU, mV, sY, sU, sV, 0} per image and group in the opponent space Y = 0.299 R + 0.587 G + 0.114 B,
    U = B - Y, V = R - Y; n == 0: zeros.  Fixed summation order: the same bits on every call, an image's row does not
    depend on its batch.  No host synchronisation."""
    bits = recolor_group_bits(groups)
    B, H, W = _recolor_inputs('region_color_stats', img, segm)
    G = len(bits)
    partial = torch.empty((B, (H + RECOLOR_STRIPE - 1) // RECOLOR_STRIPE, G, 8), device=img.device, dtype=torch.float64)
    stats = torch.empty((B, G, 8), device=img.device, dtype=torch.float64)
    check(_lib.load().t2h_region_color_stats(_p(img), int(bool(img_signed)), _p(segm), (ctypes.c_uint64 * G)(*bits), G, B, H,
                                             W, _p(partial), _p(stats), _stream()), 't2h_region_color_stats')
    return stats


def recolor_region(img, segm, groups, src_stats, dst_stats, luma=1.0, gain_max=4.0, feather=2, img_signed=False,
                   want_u8=False):
    """Moves the colour statistics of parsing-map regions onto targets (t2h_recolor_region_f32): an
    image-space operator.  img / segm / groups as region_color_stats; src_stats f64 [B, G, 8]: region_color_stats of
    this image; dst_stats f64 [B, G, 8]: the targets (another image's statistics, or src_stats with mY, mU, mV replaced
    by a plain colour's -- the gains are then 1 and pattern and shading survive).  Per group U and V are re-centred on
    the target's means and Y is shifted by luma (t.mY - s.mY); deviations are scaled by t.s / s.s within
    [1 / gain_max, gain_max].  The change fades over `feather` pixels outside a region (a tent of integer weights);
    pixels farther than that from every region keep their bits.  A group with n == 0 in either row leaves that image
    untouched there.  -> (img f32 [B, 3, H, W] in [0, 1] where touched, u8 [B, H, W, 3] or None).  No host
    synchronisation, the generator is not touched."""
    bits = recolor_group_bits(groups)
    _check_recolor_params(luma, gain_max, feather)
    B, H, W = _recolor_inputs('recolor_region', img, segm)
    G = len(bits)
    for name, st in (('src_stats', src_stats), ('dst_stats', dst_stats)):
        if not torch.is_tensor(st) or st.dtype != torch.float64 or st.device != img.device or \
                tuple(st.shape) != (B, G, 8) or not st.is_contiguous():
            got = (tuple(st.shape), st.dtype, st.device) if torch.is_tensor(st) else type(st).__name__
            raise ValueError(f'recolor_region: {name} must be a contiguous float64 [{B}, {G}, 8] tensor on {img.device} '
                             f'(region_color_stats), got {got}')
    out = torch.empty_like(img)
    u8 = torch.empty((B, H, W, 3), device=img.device, dtype=torch.uint8) if want_u8 else None
    check(_lib.load().t2h_recolor_region_f32(_p(img), int(bool(img_signed)), _p(segm), (ctypes.c_uint64 * G)(*bits), G,
                                             _p(src_stats), _p(dst_stats), float(luma), float(gain_max), int(feather),
                                             _p(out), _p(u8), B, H, W, _stream()), 't2h_recolor_region_f32')
    return out, u8


def recolor_yuv(colour):
    """(..., 3) RGB -> (..., 3) = (Y, U, V) of the recolouring's opponent space, float64 (a tensor stays on its device)"""
    c = colour.to(torch.float64) if torch.is_tensor(colour) else torch.as_tensor(colour, dtype=torch.float64)
    y = 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]
    return torch.stack([y, c[..., 2] - y, c[..., 0] - y], -1)


def recolor_rgb(yuv):
    """the inverse of recolor_yuv: (..., 3) = (Y, U, V) -> (..., 3) RGB, in the input's dtype"""
    y, u, v = yuv[..., 0], yuv[..., 1], yuv[..., 2]
    return torch.stack([y + v, y - (0.299 * v + 0.114 * u) / 0.587, y + u], -1)


def texture_map(segm, upper, lower, outer):
    """segm i64 [B,1,H,W] -> f32 mask [B,1,H,W]."""
    _chk_i64(segm, upper, lower, outer)
    B = segm.shape[0]
    hw = segm.numel() // B
    mask = torch.empty(segm.shape, device=segm.device, dtype=torch.float32)
    check(_lib.load().t2h_texture_map(_p(segm), _p(upper), _p(lower), _p(outer), _p(mask), B, hw,
                                      _stream()), 't2h_texture_map')
    return mask


def shape_attr_embed(attr, emb):
    """attr i64 [B, n_attr]; emb = dict of packed tensors (weights.pack_shape_embedder)."""
    _chk_i64(attr)
    B, n_attr = attr.shape
    out = torch.empty((B, emb['out_dim']), device=attr.device, dtype=torch.float32)
    check(_lib.load().t2h_shape_attr_embed_f32(
        _p(attr), _p(emb['cls_off']), _p(emb['w0t']), _p(emb['b0']), _p(emb['w1']), _p(emb['b1']),
        _p(emb['f0']), _p(emb['fb0']), _p(emb['f1']), _p(emb['fb1']), _p(out), B, n_attr, emb['dim'],
        emb['out_dim'], _stream()), 't2h_shape_attr_embed_f32')
    return out


def tap_bias_map(tapc, B, H, W, cout):
    """tapc f32 [B, cout, 9] -> rows [B*H*W, cout]."""
    _chk_f32(tapc)
    assert tapc.is_contiguous()
    out = torch.empty((B * H * W, cout), device=tapc.device, dtype=torch.float32)
    check(_lib.load().t2h_tap_bias_map_f32(_p(tapc), _p(out), B, H, W, cout, _stream()),
          't2h_tap_bias_map_f32')
    return out
