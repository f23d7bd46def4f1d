"""Guard-band and image-border properties of the decode / encode kernels (a plain helper module): the property code of
tests/test_gpu_decode_bands.py (the hardware) and tests/test_decode_bands_emulated.py (the kernels' source through
tests/emu), written once and parametrised by HOW TO LAUNCH (Env).  Every kernel is called through its C entry point with
buffers of the test's own, each between guard bands (tests/guard_util.py).  Properties, numbered as in
tests/test_gpu_row_counts.py:

  P1  accuracy against an fp64 reference of the same operation, with the bound the kernel's existing test uses;
  P2  every output -- the auxiliary ones too: gn_part_out, splitk_ws, GroupNorm tables and workspace, index lists --
      sits between row bands (at least one full tile of the kernel) and, where its leading dimension may exceed its
      row, between column bands, byte-identical after the launch;
  P3  every input sits between bands and, for lda / ldx > C, between columns: a run with zero bands and a run with
      poisoned bands give bitwise-equal outputs and leave the overflow word 0.  The two runs also PRE-FILL the outputs
      differently (zeros / poison), so an element of the extent that is never written shows up too.  For the 3x3
      kernels this is the border test: the top row of the first image must not see the band before it, the bottom
      row of the last image not the band after it, channels Cin .. lda - 1 must not enter a sum;
  P4  where the launch has a range guard: ONE out-of-range activated value at the last pixel of the last image and
      the last channel raises bit 0 of the overflow word;
  P5  image independence: in a batch of 3 whose middle image is entirely poison, images 0 and 2 come out bitwise equal
      to the clean run, and image 1 of the clean run bitwise equals a 1-image launch of image 1 alone."""
import ctypes
import functools
import types

import torch
import torch.nn.functional as F

import guard_util as G
from text2human_amd import ops, weights
from text2human_amd._lib import GemmArgs

F32 = torch.float32
ONE_F32 = 0x3F800000


class Env:
    """how to launch: dev = where the buffers live, lib(kernel_file) = the library that exports that file's entry
    points, stream() = the last argument of every entry point, last_error(lib) = its message"""

    def __init__(self, dev, lib, stream, last_error):
        self.dev, self.lib, self.stream, self.last_error = dev, lib, stream, last_error

    def call(self, kernel_file, name, *args):
        lib = self.lib(kernel_file)
        rc = getattr(lib, name)(*args, self.stream())
        assert rc == 0, (name, rc, self.last_error(lib))

    def forced(self, kernel_file, hook, value):
        """context manager: lib.<hook>(value), the previous setting restored on the way out"""
        return _Forced(self.lib(kernel_file), hook, value)


class _Forced:
    def __init__(self, lib, hook, value):
        self.fn, self.value = getattr(lib, hook), value

    def __enter__(self):
        self.old = self.fn(self.value)

    def __exit__(self, *exc):
        self.fn(self.old)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def f32_poison(t):
    """rows alternate between the NaN pattern (invisible to a `>=` range guard, fatal in a sum) and 1e30 (visible)"""
    G.fill_bits(t, G.F32_NAN)
    G.bits(t)[1::2] = G.F32_BIG


_POISON = {torch.float32: f32_poison, torch.float64: 0x7FF8DEADBEEF0001, torch.int16: G.SPLIT_INF, torch.int64: -7,
           torch.int32: -7, torch.uint8: 0xA5}


def _fill(t, how):
    how(t) if callable(how) else G.fill_bits(t, how)


class Buf:
    """One tensor of a launch between guard bands: `rows` rows of shape `tail`, `band` rows before and behind, and --
    cols = (c0, n) -- columns beside the logical extent.  poison False: everything zero; True: the bands, the columns
    beside the extent AND the extent hold the poison of the dtype (valid: a bit pattern / fill function instead, for
    index INPUTS, whose band values must stay in range: a test must not make an out-of-bounds read out of a read
    that should not have happened).  put() then sets the extent of an input; an output keeps its pre-fill."""

    def __init__(self, env, rows, tail, dtype, band, poison, cols=None, valid=None):
        fill = (valid if valid is not None else _POISON[dtype]) if poison else 0
        self.whole, self.rows_view = G.banded(rows, tuple(tail), dtype, env.dev, band, fill)
        self.rows, self.cols = rows, cols
        self.view = self.rows_view if cols is None else self.rows_view[:, cols[0]:cols[0] + cols[1]]
        self.snapshot = None

    def put(self, t):
        self.view.copy_(t.reshape(self.view.shape))
        return self

    def ptr(self):
        return self.view.data_ptr()

    def snap(self):
        self.snapshot = self.whole.clone()

    def check_bands(self, what):                                                                        # P2
        G.assert_bands_untouched(self.whole, G.band_of(self.whole, self.rows), self.rows, self.snapshot,
                                 *(self.cols or ()), what=what)

    def check_unwritten(self, what):
        assert torch.equal(G.bits(self.whole), G.bits(self.snapshot)), f'{what}: an input was written'

    def out(self, n_img=None):
        """the extent's bits on the CPU, [n_img, rows / n_img, ...] with n_img"""
        b = G.bits(self.view).cpu().clone()
        return b if n_img is None else b.reshape(n_img, self.rows // n_img, *b.shape[1:])


def launch_checked(env, kernel_file, name, args, outs, ins):
    """snapshots every buffer, launches, then P2 on the outputs and `unwritten` on the inputs"""
    for _, b in outs + ins:
        b.snap()
    env.call(kernel_file, name, *args)
    for what, b in outs:
        b.check_bands(f'{name}: {what}')
    for what, b in ins:
        b.check_unwritten(f'{name}: {what}')


def same(a, b, what):
    assert a.dtype == b.dtype and torch.equal(a, b), what


def properties(run, n_img, p5=True):
    """P3 and P5 of run(imgs, poison, poison_imgs=()) -> {name: bits [len(imgs), ...], 'ovf': int} (P2 is asserted
    inside run, by launch_checked) -> the clean run's outputs, for P1"""
    full = tuple(range(n_img))
    r0, r1 = run(full, False), run(full, True)
    assert r0.get('ovf', 0) == 0 and r1.get('ovf', 0) == 0, (r0.get('ovf'), r1.get('ovf'))              # P3
    for k in r0:
        if k != 'ovf':
            same(r0[k], r1[k], f'{k}: the result depends on what lies beyond the extent (or is not written)')
    if p5:                                                                                              # P5
        mid = n_img // 2
        r5 = run(full, True, (mid, ))
        r6 = run((mid, ), True)
        for k in r0:
            if k == 'ovf':
                continue
            for i in full:
                if i != mid:
                    same(r5[k][i], r0[k][i], f'{k}: image {i} depends on its (poisoned) neighbour {mid}')
            same(r6[k][0], r0[k][mid], f'{k}: image {mid} alone differs from image {mid} in a batch of {n_img}')
    return r0


def close(got_bits, ref, tol=2e-5, what=''):
    """|err| <= tol + tol |ref| (tests/test_gpu_kernels.py assert_close, tests/test_fp32_kernels_emulated.py close)"""
    got = got_bits.view(F32).double().reshape(ref.shape)
    err = (got - ref).abs()
    print(f'{what}: max err {err.max().item():.3g}')
    assert (err <= tol + tol * ref.abs()).all(), (what, err.max().item())


# ---------------------------------------------------------------------------------------------- the convolutions

_CONV_FILE = {'gemm': 'gemm.hip', 'split': 'conv_split.hip', 'halo': 'conv_halo.hip'}
_CONV_ENTRY = {'gemm': 't2h_gemm_f32', 'split': 't2h_conv_split_f32', 'halo': 't2h_conv_halo_f32'}


@functools.lru_cache(maxsize=None)
def conv_problem(n_img, cin, cout, h, w, mode, taps=9, pro=False, res_pre=0, seed=100):
    """one convolution and its fp64 reference, computed once and shared: x NHWC rows, packed weights (fp32 and split
    rows), GroupNorm tables (pro: a = swish(x * scale[img] + shift[img])), bias, residual.  res_pre 1: the residual
    goes in BEFORE a ReLU (the per-pixel bias map of the attribute channels), else it is added last."""
    p = types.SimpleNamespace(n_img=n_img, cin=cin, cout=cout, h=h, w=w, mode=mode, taps=taps, pro=pro, res_pre=res_pre)
    x = rnd(n_img, cin, h, w, seed=seed)
    k = 3 if taps == 9 else 1
    wt, p.b = rnd(cout, cin, k, k, seed=seed + 1, scale=0.1), rnd(cout, seed=seed + 2)
    p.sc, p.sh = (rnd(n_img, cin, seed=seed + 3) * 0.3 + 1).contiguous(), (rnd(n_img, cin, seed=seed + 4) * 0.3).contiguous()
    p.sc[n_img - 1, cin - 1] = 1.25                                              # (P4 divides by it)
    xin = x.double()
    if pro:
        xin = xin * p.sc.double()[:, :, None, None] + p.sh.double()[:, :, None, None]
        xin = xin * torch.sigmoid(xin)
    p.stride, p.pad, p.ups = (2, 0, 0) if mode == 'down' else (1, 1 if taps == 9 else 0, 1 if mode == 'up' else 0)
    if mode == 'up':
        xin = F.interpolate(xin, scale_factor=2.0, mode='nearest')
    if mode == 'down':
        ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), wt.double(), p.b.double(), 2, 0)
    else:
        ref = F.conv2d(xin, wt.double(), p.b.double(), 1, p.pad)
    p.ho, p.wo = ref.shape[2:]
    p.res = rnd(n_img * p.ho * p.wo, cout, seed=seed + 5)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, cout)
    p.ref = F.relu(ref + p.res.double()) if res_pre else ref + p.res.double()
    p.x_rows = x.permute(0, 2, 3, 1).reshape(n_img, h * w, cin).contiguous()
    p.w_rows = weights.pack_conv3x3(wt) if taps == 9 else wt.reshape(cout, cin).contiguous()
    p.w_split = ops.pack_split_rows_host(p.w_rows)
    p.x_split = ops.pack_split_rows_host(p.x_rows.view(-1, cin)).view(n_img, h * w, cin // 32, 2, 32)
    p.on = {}
    return p


def _on(p, env, name):
    """p.<name> on the launch's device (weights and bias: read-only, shared between launches)"""
    key = (env.dev, name)
    if key not in p.on:
        p.on[key] = getattr(p, name).to(env.dev)
    return p.on[key]


def conv_run(env, kind, p, *, band_out, lda_extra=0, ldc_extra=0, pro_extra=0, gn_stats=False, ksplit=None, spike=None):
    """-> run(imgs, poison, poison_imgs) of one convolution launch of `kind` ('gemm': t2h_gemm_f32's conv mode,
    'split': t2h_conv_split_f32 on split rows, 'halo': t2h_conv_halo_f32) with every buffer between bands.
    ksplit (gemm): None = no workspace; 0 = the library's choice, n = n slices, the workspace EXACTLY ksplit * M * N
    floats inside a banded buffer.  spike: the value x[last image, last pixel, last channel] takes (P4)."""
    cin, N, hw_in, hw_out = p.cin, p.cout, p.h * p.w, p.ho * p.wo
    c0 = ldc_extra // 2
    assert c0 % 4 == 0 and (kind != 'split' or (lda_extra == 0 and not p.pro)) and (kind != 'gemm' or not gn_stats)
    lib = env.lib(_CONV_FILE[kind])

    def run(imgs, poison, poison_imgs=()):
        n = len(imgs)
        M = n * hw_out
        band_in = max(16, 2 * p.w + 2)       # (more than an image row: a halo one row outside the batch lands here)
        if kind == 'split':
            a = Buf(env, n * hw_in, (cin // 32, 2, 32), torch.int16, band_in, poison).put(p.x_split[list(imgs)])
        else:
            a = Buf(env, n * hw_in, (cin + lda_extra, ), F32, band_in, poison, cols=(0, cin)).put(p.x_rows[list(imgs)])
        if spike is not None:
            assert kind != 'split'
            a.view[n * hw_in - 1, cin - 1] = spike
        for j, i in enumerate(imgs):
            if i in poison_imgs:             # (the whole rows of the image: its extra columns too)
                _fill(a.rows_view[j * hw_in:(j + 1) * hw_in], _POISON[a.whole.dtype])
        ins = [('A', a)]
        g = GemmArgs()
        g.A, g.B, g.bias = a.ptr(), _on(p, env, 'w_rows' if kind == 'gemm' else 'w_split').data_ptr(), _on(p, env, 'b').data_ptr()
        if p.pro:
            tabs = [Buf(env, n, (cin + pro_extra, ), F32, 4, poison, cols=(0, cin)).put(t[list(imgs)]) for t in (p.sc, p.sh)]
            g.pro_scale, g.pro_shift, g.pro_ld, g.pro_act = tabs[0].ptr(), tabs[1].ptr(), cin + pro_extra, 1
            ins += [('pro_scale', tabs[0]), ('pro_shift', tabs[1])]
        res = Buf(env, M, (N + 8, ), F32, 16, poison, cols=(4, N)).put(p.res.view(p.n_img, hw_out, N)[list(imgs)])
        ins.append(('residual', res))
        c = Buf(env, M, (N + ldc_extra, ), F32, band_out, poison, cols=(c0, N))
        outs = [('C', c)]
        g.C, g.residual = c.ptr(), res.ptr()
        g.M, g.N, g.K = M, N, p.taps * cin
        g.lda, g.ldb, g.ldc, g.ldr = (0 if kind == 'split' else cin + lda_extra), (g.K if kind == 'gemm' else 0), N + ldc_extra, N + 8
        g.a_mode, g.epi_act, g.alpha, g.res_pre, g.batch = 1, (2 if p.res_pre else 0), 1.0, p.res_pre, 1
        g.Hin, g.Win, g.Cin, g.Hout, g.Wout = p.h, p.w, cin, p.ho, p.wo
        g.stride, g.pad, g.ups = p.stride, p.pad, p.ups
        part = ws = None
        if gn_stats:
            chunks = hw_out // 128
            part = Buf(env, n * chunks * 2, (N, ), torch.float64, max(8, 2 * chunks), poison)
            g.gn_part_out = part.ptr()
            outs.append(('gn_part_out', part))
        if ksplit is not None:
            g.splitk_ws, g.splitk_ws_floats, g.ksplit = c.ptr(), 1 << 40, ksplit          # (the query reads no memory)
            ks = lib.t2h_gemm_ksplit(ctypes.byref(g))
            assert ks >= 1 and (ksplit == 0 or ks == ksplit), (ks, ksplit)
            ws = Buf(env, ks * M, (N, ), F32, max(16, M), poison)
            g.splitk_ws, g.splitk_ws_floats = ws.ptr(), ks * M * N
            outs.append(('splitk_ws', ws))
        ovf = torch.zeros(1, dtype=torch.int32, device=env.dev)
        args = (ctypes.byref(g), ovf.data_ptr()) if kind == 'halo' else (ctypes.byref(g), )
        launch_checked(env, _CONV_FILE[kind], _CONV_ENTRY[kind], args, outs, ins)
        r = {'C': c.out(n), 'ovf': int(ovf.cpu()[0])}
        if part is not None:
            r['gn_part_out'] = part.out(n)
        return r

    return run


def check_conv(p, r0, gn_stats=False, what=''):
    """P1 of a convolution: 2e-5 + 2e-5 |ref| (tests/test_gpu_kernels.py, test_gpu_conv_split.py, test_gpu_conv_halo.py);
    the GroupNorm partials are the sums of the values the launch wrote, over every pixel exactly once (1e-9 relative:
    tests/test_conv_halo_emulated.py)"""
    close(r0['C'], p.ref.view(p.n_img, -1, p.cout), what=what)
    if gn_stats:
        out = r0['C'].view(F32).double()
        part = r0['gn_part_out'].view(torch.float64).view(p.n_img, -1, 2, p.cout)
        for j, want in enumerate((out.sum(1), (out * out).sum(1))):
            assert (part[:, :, j].sum(1) - want).abs().max().item() < 1e-9 * max(1.0, float(want.abs().max()))


def conv_case(env, kind, p, p4=False, p5=True, **kw):
    """P1 .. P5 of one convolution"""
    r0 = properties(conv_run(env, kind, p, **kw), p.n_img, p5=p5)
    check_conv(p, r0, kw.get('gn_stats', False), what=f'{kind} {p.mode}')
    if p4:                                                                                              # P4
        v = 1.0e5 / float(p.sc[p.n_img - 1, p.cin - 1]) if p.pro else 1.0e5
        r4 = conv_run(env, kind, p, spike=v, **kw)(tuple(range(p.n_img)), True)
        assert r4['ovf'] & 1, 'one out-of-range value at the last pixel / last channel went unnoticed'
    return r0


def plain_gemm_into_the_right_half(env):
    """t2h_gemm_f32, plain, as engine.py writes a GEMM into cat[:, cs:] of a 2 * cs-wide buffer: M = 130, N = 40 and
    K = 96 (the issue's K = 72 is no multiple of 32: rejected), A with lda = K + 8.  The left half stays byte-identical."""
    M, N, K = 130, 40, 96
    a, w, bias = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.2), rnd(N, seed=3)
    ref = a.double() @ w.double().t() + bias.double()

    def run(imgs, poison, poison_imgs=()):
        ab = Buf(env, M, (K + 8, ), F32, 16, poison, cols=(0, K)).put(a)
        cb = Buf(env, M, (2 * N, ), F32, 128, poison, cols=(N, N))
        wd, bd = w.to(env.dev), bias.to(env.dev)
        g = GemmArgs()
        g.A, g.B, g.C, g.bias = ab.ptr(), wd.data_ptr(), cb.ptr(), bd.data_ptr()
        g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.alpha, g.batch = M, N, K, K + 8, K, 2 * N, 1.0, 1
        launch_checked(env, 'gemm.hip', 't2h_gemm_f32', (ctypes.byref(g), ), [('C', cb)], [('A', ab)])
        return {'C': cb.out()}

    close(properties(run, 1, p5=False)['C'], ref, what='plain gemm')


# ---------------------------------------------------------------------------------------------- GroupNorm


def gn_apply_split_case(env):
    """t2h_gn_apply_split_f32: 3 images x 37 pixels, C = 96, ldx = tbl_ld = 128"""
    n_img, hw, C, ld = 3, 37, 96, 128
    x = rnd(n_img, hw, C, seed=11) * 1.5
    sc, sh = rnd(n_img, C, seed=12) * 0.3 + 1, rnd(n_img, C, seed=13) * 0.3
    sc[n_img - 1, C - 1] = 1.25                                                  # (P4 divides by it)
    act = x.double() * sc.double()[:, None] + sh.double()[:, None]
    act = act * torch.sigmoid(act)

    def make(tables, spike=None):
        def run(imgs, poison, poison_imgs=()):
            n = len(imgs)
            xb = Buf(env, n * hw, (ld, ), F32, 16, poison, cols=(0, C)).put(x[list(imgs)])
            if spike is not None:
                xb.view[n * hw - 1, C - 1] = spike
            for j, i in enumerate(imgs):
                if i in poison_imgs:
                    f32_poison(xb.rows_view[j * hw:(j + 1) * hw])
            ins, tp = [('x', xb)], (None, None)
            if tables:
                tabs = [Buf(env, n, (ld, ), F32, 4, poison, cols=(0, C)).put(t[list(imgs)]) for t in (sc, sh)]
                ins += [('scale', tabs[0]), ('shift', tabs[1])]
                tp = (tabs[0].ptr(), tabs[1].ptr())
            ob = Buf(env, n * hw, (C // 32, 2, 32), torch.int16, 16, poison)
            ovf = torch.zeros(1, dtype=torch.int32, device=env.dev)
            launch_checked(env, 'norm.hip', 't2h_gn_apply_split_f32',
                           (xb.ptr(), ld, *tp, ld if tables else 0, ob.ptr(), n * hw, hw, C, int(tables), ovf.data_ptr()),
                           [('out_split', ob)], ins)
            return {'rows': ob.out(n), 'ovf': int(ovf.cpu()[0])}
        return run

    r0 = properties(make(True), n_img)
    got = ops.unsplit_rows_host(r0['rows'].reshape(-1), n_img * hw, C).double().view(n_img, hw, C)
    assert ((got - act).abs() <= 2e-6 + 2e-6 * act.abs()).all()                  # P1 (tests/test_decode_convs_emulated.py)
    r0 = properties(make(False), n_img)                                           # no tables: bitwise the host split
    same(r0['rows'].reshape(-1), ops.pack_split_rows_host(x.view(-1, C)).reshape(-1), 'plain split')
    full = tuple(range(n_img))
    assert make(False, spike=1.0e5)(full, True)['ovf'] == 1                                             # P4
    assert make(True, spike=1.0e5 / float(sc[n_img - 1, C - 1]))(full, True)['ovf'] == 1


def _gn_tables_ref(x, gamma, beta, groups, eps):
    n_img, hw, C = x.shape
    xg = x.double().view(n_img, hw, groups, C // groups)
    mean = xg.mean((1, 3), keepdim=True).expand(n_img, 1, groups, C // groups).reshape(n_img, C)
    var = xg.var((1, 3), unbiased=False, keepdim=True).expand(n_img, 1, groups, C // groups).reshape(n_img, C)
    scale = gamma.double() / torch.sqrt(var + eps)
    return scale, beta.double() - mean * scale


def groupnorm_tables_case(env):
    """t2h_groupnorm_tables_f32: hw = 130, n_img = 3, ldx = C + 32; C = 128 (4 channels per group), the nearest count to
    the issue's 96 that the pass over the tensor accepts (C / 4 must divide 256; 96 is served by the finalize below)."""
    n_img, hw, C, groups, eps = 3, 130, 128, 32, 1e-6
    x = rnd(n_img, hw, C, seed=21) * 1.7 + 0.4
    gamma, beta = rnd(C, seed=22) * 0.3 + 1, rnd(C, seed=23) * 0.2
    lib = env.lib('norm.hip')

    def run(imgs, poison, poison_imgs=()):
        n = len(imgs)
        xb = Buf(env, n * hw, (C + 32, ), F32, 16, poison, cols=(0, C)).put(x[list(imgs)])
        for j, i in enumerate(imgs):
            if i in poison_imgs:
                f32_poison(xb.rows_view[j * hw:(j + 1) * hw])
        sb, tb = (Buf(env, n, (C, ), F32, 4, poison) for _ in range(2))
        assert lib.t2h_groupnorm_workspace_bytes(n, hw, C) == n * 2 * C * 8        # (one 1024-pixel chunk per image)
        wsb = Buf(env, n * 2, (C, ), torch.float64, 4, poison)
        gd, bd = gamma.to(env.dev), beta.to(env.dev)
        launch_checked(env, 'norm.hip', 't2h_groupnorm_tables_f32',
                       (xb.ptr(), C + 32, gd.data_ptr(), bd.data_ptr(), sb.ptr(), tb.ptr(), n, hw, C, groups, eps, wsb.ptr()),
                       [('scale', sb), ('shift', tb), ('workspace', wsb)], [('x', xb)])
        return {'scale': sb.out(n), 'shift': tb.out(n), 'workspace': wsb.out(n)}

    r0 = properties(run, n_img)
    want = _gn_tables_ref(x, gamma, beta, groups, eps)
    for k, wv in zip(('scale', 'shift'), want):                                   # P1 (tests/test_gpu_kernels.py: 1e-5)
        assert (r0[k].view(F32).double().view(n_img, C) - wv).abs().max().item() < 1e-5


def groupnorm_finalize_case(env):
    """t2h_groupnorm_finalize_f32 from per-128-pixel partials: C = 96 (3 channels per group), 2 chunks, n_img = 3"""
    n_img, hw, C, groups, eps, chunks = 3, 256, 96, 32, 1e-6, 2
    x = rnd(n_img, hw, C, seed=24) * 1.7 + 0.4
    gamma, beta = rnd(C, seed=25) * 0.3 + 1, rnd(C, seed=26) * 0.2
    xc = x.double().view(n_img, chunks, 128, C)
    part = torch.stack([xc.sum(2), (xc * xc).sum(2)], 2).contiguous()             # [n_img, chunks, 2, C]

    def run(imgs, poison, poison_imgs=()):
        n = len(imgs)
        pb = Buf(env, n * chunks * 2, (C, ), torch.float64, 8, poison).put(part[list(imgs)])
        for j, i in enumerate(imgs):
            if i in poison_imgs:
                G.fill_bits(pb.view[j * chunks * 2:(j + 1) * chunks * 2], _POISON[torch.float64])
        sb, tb = (Buf(env, n, (C, ), F32, 4, poison) for _ in range(2))
        gd, bd = gamma.to(env.dev), beta.to(env.dev)
        launch_checked(env, 'norm.hip', 't2h_groupnorm_finalize_f32',
                       (pb.ptr(), chunks, gd.data_ptr(), bd.data_ptr(), sb.ptr(), tb.ptr(), n, hw, C, groups, eps),
                       [('scale', sb), ('shift', tb)], [('part', pb)])
        return {'scale': sb.out(n), 'shift': tb.out(n)}

    r0 = properties(run, n_img)
    for k, wv in zip(('scale', 'shift'), _gn_tables_ref(x, gamma, beta, groups, eps)):
        assert (r0[k].view(F32).double().view(n_img, C) - wv).abs().max().item() < 1e-5


# ---------------------------------------------------------------------------------------------- conv_out, AttnBlock


def conv_small_case(env, cout, pro):
    """t2h_conv3x3_small_f32: 13 x 37, cin = 32, ldx = 64, ldo = 8 (the decoder's output row is read with a stride by
    t2h_image_epilogue), tables with tbl_ld = 48"""
    p = conv_problem(3, 32, cout, 13, 37, 'same', pro=pro, seed=300 + cout)
    hw, cin = 13 * 37, 32

    def run(imgs, poison, poison_imgs=()):
        n = len(imgs)
        xb = Buf(env, n * hw, (64, ), F32, 2 * 37 + 2, poison, cols=(0, cin)).put(p.x_rows[list(imgs)])
        for j, i in enumerate(imgs):
            if i in poison_imgs:
                f32_poison(xb.rows_view[j * hw:(j + 1) * hw])
        ins, tp = [('x', xb)], (None, None)
        if pro:
            tabs = [Buf(env, n, (48, ), F32, 4, poison, cols=(0, cin)).put(t[list(imgs)]) for t in (p.sc, p.sh)]
            ins += [('scale', tabs[0]), ('shift', tabs[1])]
            tp = (tabs[0].ptr(), tabs[1].ptr())
        ob = Buf(env, n * hw, (8, ), F32, 8 * 37, poison, cols=(4, cout))          # (a tile is 8 image rows)
        launch_checked(env, 'conv_small.hip', 't2h_conv3x3_small_f32',
                       (xb.ptr(), 64, _on(p, env, 'w_rows').data_ptr(), _on(p, env, 'b').data_ptr(), *tp, 48 if pro else 0,
                        int(pro), ob.ptr(), 8, n, 13, 37, cin, cout), [('out', ob)], ins)
        return {'out': ob.out(n)}

    r0 = properties(run, 3)
    close(r0['out'], (p.ref - p.res.double()).view(3, hw, cout), what=f'conv_small cout={cout}')   # (no residual here)


def spatial_attention_case(env):
    """t2h_spatial_attention_f32: N = 96, C = 256, n_img = 3, ld = 3C + 32, ldo = C + 32"""
    n_img, N, C = 3, 96, 256
    qkv = rnd(n_img, N, 3 * C, seed=31) * 0.5
    scale = float(int(C) ** -0.5)
    q, k, v = (t.double() for t in qkv.split(C, dim=2))
    ref = torch.softmax(torch.bmm(q, k.transpose(1, 2)) * scale, dim=2) @ v

    def run(imgs, poison, poison_imgs=()):
        n = len(imgs)
        xb = Buf(env, n * N, (3 * C + 32, ), F32, 32, poison, cols=(0, 3 * C)).put(qkv[list(imgs)])
        for j, i in enumerate(imgs):
            if i in poison_imgs:
                f32_poison(xb.rows_view[j * N:(j + 1) * N])
        ob = Buf(env, n * N, (C + 32, ), F32, 32, poison, cols=(16, C))            # (a workgroup is 32 queries)
        launch_checked(env, 'spatial_attn.hip', 't2h_spatial_attention_f32',
                       (xb.ptr(), 3 * C + 32, ob.ptr(), C + 32, n, N, C, scale), [('out', ob)], [('qkv', xb)])
        return {'out': ob.out(n)}

    close(properties(run, n_img)['out'], ref, what='spatial attention')


# ---------------------------------------------------------------------------------------------- quantizers

N_ROWS, N_E, N_BOOKS = 3 * 37, 37, 3


def _argmin_check(got, z, book, what):
    """exact equality with the fp64 argmin of the EXPANDED distance wherever best and second best are further apart
    than the margin of tests/test_gpu_kernels.py test_vq_l2_argmin_first_min_and_margin (1e-4)"""
    dist = (z.double() ** 2).sum(1, keepdim=True) + (book.double() ** 2).sum(1) - 2 * z.double() @ book.double().t()
    s = dist.sort(1).values
    clear = (s[:, 1] - s[:, 0]) >= 1e-4
    assert clear.float().mean().item() > 0.9, what
    same(got[clear], dist.argmin(1)[clear], what)


def _hit_fill(row):
    """band fill of z: every band row EQUALS a codebook entry -- reading it changes no distance anywhere, but the row
    it would be quantised for lies in the index list's band (P2)"""
    def fill(whole):
        whole.copy_(row.to(whole.device).expand_as(whole))
    return fill


def vq_l2_argmin_case(env):
    """t2h_vq_l2_argmin_f32: n = 111, n_e = 37 (no multiple of the 256-code LDS tile), d = 64 (d = 256 is not served:
    32 / 64)"""
    d = 64
    z, book = rnd(N_ROWS, d, seed=41), rnd(N_E, d, seed=42)
    z[5] = book[11]

    def run(imgs, poison, poison_imgs=()):
        zb = Buf(env, N_ROWS, (d, ), F32, 32, poison, valid=_hit_fill(book[7])).put(z)
        ib = Buf(env, N_ROWS, (), torch.int64, 32, poison)                         # (a workgroup is 32 rows)
        bd = book.to(env.dev)
        launch_checked(env, 'vq.hip', 't2h_vq_l2_argmin_f32', (zb.ptr(), bd.data_ptr(), ib.ptr(), N_ROWS, N_E, d),
                       [('idx', ib)], [('z', zb)])
        return {'idx': ib.out()}

    got = properties(run, 1, p5=False)['idx']
    assert int(got[5]) == 11
    _argmin_check(got, z, book, 'vq_l2_argmin')


def vq_argmin_tex_case(env, fold, n=N_ROWS, n_e=N_E):
    """t2h_vq_argmin_tex_f32, d = 256, n rows (no multiple of the 4 rows of a workgroup), n_e codes (no multiple of the 4
    codes of a step): plain rows, or (fold) the 2x2 patches of an NHWC map [n / 37, 74, 2, 64]"""
    d, fh, fw = 256, (37 if fold else 0), (1 if fold else 0)
    assert n % 37 == 0
    z, books = rnd(n, d, seed=43), rnd(N_BOOKS, n_e, d, seed=44)
    tex = torch.arange(n) % N_BOOKS
    tex = tex[torch.randperm(n, generator=torch.Generator().manual_seed(45))].contiguous()
    if fold:   # row (b, i, j) = patch [c, kh, kw] of the map
        zmap = z.view(n // 37, fh, fw, d // 4, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n * 4, d // 4).contiguous()
    else:
        zmap = z

    def run(imgs, poison, poison_imgs=()):
        zb = Buf(env, zmap.shape[0], (zmap.shape[1], ), F32, 16, poison, valid=_hit_fill(books[0, 3, :zmap.shape[1]])).put(zmap)
        tb = Buf(env, n, (), torch.int64, 16, poison, valid=1).put(tex)
        lb = Buf(env, N_BOOKS, (n, ), torch.int64, 2, poison)
        bd = books.to(env.dev)
        launch_checked(env, 'vq.hip', 't2h_vq_argmin_tex_f32',
                       (zb.ptr(), bd.data_ptr(), tb.ptr(), lb.ptr(), n, N_BOOKS, n_e, d, fh, fw),
                       [('idx_lists', lb)], [('z', zb), ('tex', tb)])
        return {'lists': lb.out()}

    lists = properties(run, 1, p5=False)['lists']
    for hd in range(N_BOOKS):
        rows = (tex == hd).nonzero().flatten()
        assert (lists[hd][tex != hd] == -1).all() and len(rows)
        _argmin_check(lists[hd][rows], z[rows], books[hd], f'vq_argmin_tex head {hd}')


def codebook_gathers_case(env):
    """t2h_codebook_gather_tex_f32 (e_dim = 256) and t2h_codebook_gather_fold_f32 (B = 3, h = 37, w = 1, C = 64)"""
    g = torch.Generator().manual_seed(46)
    books = rnd(N_BOOKS, N_E, 256, seed=47)
    tex = torch.randint(0, N_BOOKS, (N_ROWS, ), generator=g)
    pick = torch.randint(0, N_E, (N_ROWS, ), generator=g)
    lists = torch.full((N_BOOKS, N_ROWS), -1, dtype=torch.int64)
    lists[tex, torch.arange(N_ROWS)] = pick
    ent = books[tex, pick]

    def make(fold):
        def run(imgs, poison, poison_imgs=()):
            lb = Buf(env, N_BOOKS, (N_ROWS, ), torch.int64, 2, poison, valid=1).put(lists)
            tb = Buf(env, N_ROWS, (), torch.int64, 16, poison, valid=1).put(tex)
            bd = books.to(env.dev)
            if fold:
                ob = Buf(env, 3 * 74 * 2, (64, ), F32, 16, poison)
                args = (lb.ptr(), tb.ptr(), bd.data_ptr(), ob.ptr(), 3, 37, 1, N_BOOKS, N_E, 64)
            else:
                ob = Buf(env, N_ROWS, (256, ), F32, 16, poison)
                args = (lb.ptr(), tb.ptr(), bd.data_ptr(), ob.ptr(), N_ROWS, N_BOOKS, N_E, 256)
            launch_checked(env, 'vq.hip', 't2h_codebook_gather_fold_f32' if fold else 't2h_codebook_gather_tex_f32', args,
                           [('out', ob)], [('idx_lists', lb), ('tex', tb)])
            return {'out': ob.out()}
        return run

    same(properties(make(False), 1, p5=False)['out'], G.bits(ent), 'codebook_gather_tex')               # P1: exact
    want = F.fold(ent.view(3, 37, 256).permute(0, 2, 1), (74, 2), kernel_size=2, stride=2).permute(0, 2, 3, 1).contiguous()
    same(properties(make(True), 1, p5=False)['out'], G.bits(want.view(-1, 64)), 'codebook_gather_fold')


def routed_head_argmax_case(env, n=N_ROWS):
    """t2h_routed_head_argmax: n rows (111), 3 heads, Cf = 32, 37 classes, ldf = 3 * 32 + 32"""
    n_heads, Cf, n_class = N_BOOKS, 32, N_E
    g = torch.Generator().manual_seed(48)
    feat = rnd(n, n_heads * Cf, seed=49)
    w, b = rnd(n_heads, n_class, Cf, seed=50) * 0.3, rnd(n_heads, n_class, seed=51) * 0.1
    tex = torch.randint(0, n_heads, (n, ), generator=g)

    def run(imgs, poison, poison_imgs=()):
        fb = Buf(env, n, (n_heads * Cf + 32, ), F32, 16, poison, cols=(0, n_heads * Cf)).put(feat)
        tb = Buf(env, n, (), torch.int64, 16, poison, valid=1).put(tex)
        lb = Buf(env, n_heads, (n, ), torch.int64, 2, poison)
        wd, bd = w.to(env.dev), b.to(env.dev)
        launch_checked(env, 'vq.hip', 't2h_routed_head_argmax',
                       (fb.ptr(), n_heads * Cf + 32, wd.data_ptr(), bd.data_ptr(), tb.ptr(), lb.ptr(), n, n_heads, Cf, n_class),
                       [('out_lists', lb)], [('feat', fb), ('tex', tb)])
        return {'lists': lb.out()}

    lists = properties(run, 1, p5=False)['lists']
    for r in range(n):   # (margin and form of tests/test_layout_kernels_emulated.py)
        hd = int(tex[r])
        sc = w[hd].double() @ feat[r, hd * Cf:(hd + 1) * Cf].double() + b[hd].double()
        top = sc.topk(2)
        assert (lists[:, r] >= 0).sum() == 1 and (lists[:, r] == -1).sum() == n_heads - 1
        if top.values[0] - top.values[1] > 1e-4:
            assert lists[hd, r] == top.indices[0]


# ---------------------------------------------------------------------------------------------- layout kernels

LB, LH, LW = 3, 6, 10


def _per_image(env, file, name, x, in_tail, in_cols, out_rows, out_tail, out_dtype, args, band_in=16, band_out=16,
               out_cols=None):
    """run() of a layout kernel with one input x [B, rows per image, *] and one output (out_rows per image)"""
    def run(imgs, poison, poison_imgs=()):
        n, rpi = len(imgs), x.shape[1]
        xb = Buf(env, n * rpi, in_tail, x.dtype, band_in, poison, cols=in_cols).put(x[list(imgs)])
        for j, i in enumerate(imgs):
            if i in poison_imgs:
                _fill(xb.rows_view[j * rpi:(j + 1) * rpi], _POISON[x.dtype])
        ob = Buf(env, n * out_rows, out_tail, out_dtype, band_out, poison, cols=out_cols)
        launch_checked(env, file, name, args(xb, ob, n), [('out', ob)], [('in', xb)])
        return {'out': ob.out(n)}
    return run


def layout_cases(env):
    """csrc/misc.hip at B = 3, H = 6, W = 10, C = 19 (20 where the kernel needs C % 4 == 0): exact operations, P1 bitwise
    against torch on the CPU (bilinear: the 1e-6 of tests/test_gpu_kernels.py -- its weighted sums round)"""
    B, H, W, HW = LB, LH, LW, LH * LW
    # NCHW -> NHWC with cpad = 24 > C = 19
    x = rnd(B, 19, HW, seed=61)
    run = _per_image(env, 'misc.hip', 't2h_nchw_to_nhwc_f32', x, (HW, ), None, HW, (24, ), F32,
                     lambda xb, ob, n: (xb.ptr(), ob.ptr(), n, 19, HW, 24), out_cols=(0, 19), band_out=32)
    same(properties(run, B)['out'], G.bits(x.permute(0, 2, 1).contiguous()), 'nchw_to_nhwc')
    # NHWC (ldx = 24) -> NCHW
    xr = x.permute(0, 2, 1).contiguous()
    run = _per_image(env, 'misc.hip', 't2h_nhwc_to_nchw_f32', xr, (24, ), (0, 19), 19, (HW, ), F32,
                     lambda xb, ob, n: (xb.ptr(), 24, ob.ptr(), n, 19, HW), band_in=32, band_out=32)
    same(properties(run, B)['out'], G.bits(x), 'nhwc_to_nchw')
    # MaxPool2d(2), C = 20, ldx = 24
    x4 = rnd(B, 20, H, W, seed=62)
    rows = x4.permute(0, 2, 3, 1).reshape(B, HW, 20).contiguous()
    run = _per_image(env, 'misc.hip', 't2h_maxpool2_nhwc_f32', rows, (24, ), (0, 20), HW // 4, (20, ), F32,
                     lambda xb, ob, n: (xb.ptr(), 24, ob.ptr(), n, H, W, 20), band_in=2 * W + 2, band_out=64)
    same(properties(run, B)['out'], G.bits(F.max_pool2d(x4, 2).permute(0, 2, 3, 1).reshape(B, HW // 4, 20).contiguous()), 'maxpool2')
    # bilinear x2, C = 20
    run = _per_image(env, 'misc.hip', 't2h_bilinear_up2_nhwc_f32', rows, (20, ), None, 4 * HW, (20, ), F32,
                     lambda xb, ob, n: (xb.ptr(), ob.ptr(), n, H, W, 20), band_in=2 * W + 2, band_out=64)
    want = F.interpolate(x4.double(), scale_factor=2, mode='bilinear', align_corners=False).permute(0, 2, 3, 1).reshape(B, 4 * HW, 20)
    close(properties(run, B)['out'], want, tol=1e-6, what='bilinear_up2')
    # one-hot, 19 classes in Cpad = 20 columns; the band of segm holds a valid class
    segm = torch.randint(0, 19, (B, HW), generator=torch.Generator().manual_seed(63)).float()

    def run(imgs, poison, poison_imgs=()):
        sb = Buf(env, B * HW, (), F32, 16, poison, valid=ONE_F32).put(segm)
        ob = Buf(env, B * HW, (20, ), F32, 64, poison)
        launch_checked(env, 'misc.hip', 't2h_onehot_nhwc_f32', (sb.ptr(), ob.ptr(), B * HW, 19, 20), [('out', ob)], [('segm', sb)])
        return {'out': ob.out()}
    want = torch.zeros(B * HW, 20)
    want[:, :19] = F.one_hot(segm.long().view(-1), 19).float()
    same(properties(run, 1, p5=False)['out'], G.bits(want), 'onehot')
    # channel argmax, ld = 24 > n = 19

    def run(imgs, poison, poison_imgs=()):
        xb = Buf(env, B * HW, (24, ), F32, 16, poison, cols=(0, 19)).put(xr)
        ob = Buf(env, B * HW, (), torch.int64, 256, poison)
        launch_checked(env, 'misc.hip', 't2h_argmax_rows_f32', (xb.ptr(), 24, ob.ptr(), B * HW, 19), [('out', ob)], [('x', xb)])
        return {'out': ob.out()}
    same(properties(run, 1, p5=False)['out'], xr.reshape(B * HW, 19).argmax(1), 'argmax_rows')
    # image epilogue: dec rows with ldd = 8, both outputs banded
    dec = rnd(B, HW, 3, seed=64) * 0.8
    dec[0, 0], dec[1, 1] = torch.tensor([-1.0, 1.0, 0.0]), torch.tensor([-3.0, 3.0, 1.0 / 255.0 - 1.0])

    def run(imgs, poison, poison_imgs=()):
        n = len(imgs)
        db = Buf(env, n * HW, (8, ), F32, 16, poison, cols=(0, 3)).put(dec[list(imgs)])
        for j, i in enumerate(imgs):
            if i in poison_imgs:
                f32_poison(db.rows_view[j * HW:(j + 1) * HW])
        ib = Buf(env, n * 3, (HW, ), F32, 8, poison)
        ub = Buf(env, n * HW, (3, ), torch.uint8, 256, poison)
        launch_checked(env, 'misc.hip', 't2h_image_epilogue', (db.ptr(), 8, ib.ptr(), ub.ptr(), n, HW),
                       [('img_nchw', ib), ('img_u8', ub)], [('dec', db)])
        return {'img': ib.out(n), 'u8': ub.out(n)}
    r0 = properties(run, B)
    want = ((dec + 1) / 2).clamp(0, 1)
    same(r0['img'], G.bits(want.permute(0, 2, 1).contiguous()), 'image_epilogue f32')
    same(r0['u8'], want.mul(255).add(0.5).clamp(0, 255).to(torch.uint8), 'image_epilogue u8')
    # tap bias map: the taps inside the image, added in tap order
    tapc = rnd(B, 19, 9, seed=65)
    run = _per_image(env, 'misc.hip', 't2h_tap_bias_map_f32', tapc, (9, ), None, HW, (19, ), F32,
                     lambda xb, ob, n: (xb.ptr(), ob.ptr(), n, H, W, 19), band_out=64)
    want = torch.zeros(B, H, W, 19)
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    for dy in range(3):
        for dx in range(3):
            inside = ((ys + dy - 1 >= 0) & (ys + dy - 1 < H) & (xs + dx - 1 >= 0) & (xs + dx - 1 < W)).float()
            want = want + inside.view(1, H, W, 1) * tapc[:, :, dy * 3 + dx].view(B, 1, 1, 19)
    same(properties(run, B)['out'], G.bits(want.view(B, HW, 19)), 'tap_bias_map')
