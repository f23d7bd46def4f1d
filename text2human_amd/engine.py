"""Host-side composition of the HIP kernels into the stages of the sampling
path: segm tokenizer (T), index sampler (S),
feed-forward index refinement (R), hierarchical decode (D), pose front-end (P).

Everything here is batched over images (the reference decodes one image at a
time, models/sample_model.py:220; every op is per-sample so batching is exact)
and keeps activations as NHWC pixel rows [B*H*W, C] / token rows [B*T, C] in
HBM.  PyTorch only allocates tensors and provides the stream.
"""
import contextlib
import gc
import numbers
import os
import weakref

import numpy as np
import torch

from . import _lib, ops, options, schedule
from .ops import ACT_GELU, ACT_NONE, ACT_RELU, PRO_NONE, PRO_SWISH


# ---------------------------------------------------------------- VQGAN stacks


class VQGANStack:
    """Encoder / Decoder / DecoderRes forward over packed params `P` (see
    weights.pack_vqgan) under prefix `name`."""

    def __init__(self, P, name, desc):
        self.P, self.name, self.desc = P, name, desc
        self.use_split = True  # False: exact-fp32 convolutions even if split-row weights were packed (A/B, bench parity)
        # the decoders' AttnBlocks (N = 512 .. 8192 positions) MAY run flash-style when the N x N score tensor is too
        # large to allocate (attnblock); the encoders' (tokenizer: an argmin decision pinned to golden tokens) always
        # keep the materialised bmm -> softmax -> bmm form
        self.flash_attn = False

    def _ws(self, key, hw, mode='same'):
        """Split-row weights of `key` if the stack was packed with them (weights.add_split_conv_weights)
        and t2h_conv_split_f32 serves the shape, else None (-> exact-fp32 kernel)."""
        ws = self.P.t.get(key + 's') if self.use_split else None
        return ws if ws is not None and ops.conv_split_ok(hw, mode) else None

    def _gn(self, x, pfx, n_img, hw):
        P = self.P
        return ops.groupnorm_tables(x, P[f'{pfx}.g'], P[f'{pfx}.b'], n_img, hw)

    def _norm_conv3x3(self, x, norm, conv, n_img, h, w, mode='same', residual=None):
        """conv(swish(GroupNorm(x))) (+ residual): GroupNorm + swish fused into the conv's operand
        staging (exact-fp32 kernel), or -- split path -- applied by ONE elementwise pass that also
        writes the two fp16 planes the split-precision conv reads (norm None: plain conv)."""
        P = self.P
        cin = P[f'{conv}.w'].shape[1] // 9
        cout = P[f'{conv}.w'].shape[0]
        hw_out = h * w * (4 if mode == 'up' else 1)
        ws = self._ws(f'{conv}.w', hw_out, mode)
        pro = self._gn(x, norm, n_img, h * w) if norm is not None else None
        if (ws is not None and x.stride(0) * h * w * 4 < 2**31
                and ops.conv_halo_ok(n_img, h * (2 if mode == 'up' else 1), w * (2 if mode == 'up' else 1), cin, cout, mode)):
            # large levels: GroupNorm apply + swish + split happen while the 18 x 18-pixel halo of a 16 x 16 tile is
            # staged (csrc/conv_halo.hip) -- no elementwise pass, every input pixel read 1.27x instead of 9x
            return ops.conv_halo(x, ws, n_img, h, w, cin, cout, bias=P[f'{conv}.b'], residual=residual, mode=mode,
                                 pro=pro, gn_stats=cout <= 1024)
        if ws is not None:
            xs = ops.gn_apply_split(x, *(pro or (None, None)), rows_per_img=h * w,
                                    act=PRO_SWISH if pro is not None else PRO_NONE)
            return ops.conv_split(xs, ws, n_img, h, w, cin, cout, bias=P[f'{conv}.b'], residual=residual, mode=mode,
                                  gn_stats=cout <= 1024)
        if residual is None and ops.conv3x3_small_ok(cin, cout, mode):  # conv_out: 3 output channels
            return ops.conv3x3_small(x, P[f'{conv}.w'], n_img, h, w, cin, bias=P[f'{conv}.b'],
                                     pro=(pro[0], pro[1], PRO_SWISH) if pro is not None else None)
        return ops.conv3x3(x, P[f'{conv}.w'], n_img, h, w, cin, bias=P[f'{conv}.b'], mode=mode, residual=residual,
                           pro=(pro[0], pro[1], PRO_SWISH) if pro is not None else None)

    def _conv1x1(self, x, key, n_rows_img, pro=None, residual=None):
        """1x1 convolution of pixel rows (pro = GroupNorm tables applied without activation)."""
        P = self.P
        ws = self._ws(f'{key}.w', n_rows_img)
        if ws is not None:
            xs = ops.gn_apply_split(x, *(pro or (None, None)), rows_per_img=n_rows_img)
            cout, cin = P[f'{key}.w'].shape
            return ops.conv_split(xs, ws, x.shape[0] // n_rows_img, n_rows_img, 1, cin, cout, taps=1,
                                  bias=P[f'{key}.b'], residual=residual, gn_stats=cout <= 1024)
        return ops.gemm(x, P[f'{key}.w'], bias=P[f'{key}.b'], residual=residual,
                        pro=(pro[0], pro[1], n_rows_img, PRO_NONE) if pro is not None else None)

    def resblock(self, x, pfx, n_img, h, w):
        """ResnetBlock.forward (vqgan_arch.py:597-617): GroupNorm + swish go with the following conv's
        operand, bias + skip into its epilogue."""
        t = self._norm_conv3x3(x, f'{pfx}.norm1', f'{pfx}.conv1', n_img, h, w)
        skip = x
        if f'{pfx}.nin.w' in self.P:
            skip = self._conv1x1(x, f'{pfx}.nin', h * w)
        return self._norm_conv3x3(t, f'{pfx}.norm2', f'{pfx}.conv2', n_img, h, w, residual=skip)

    def attnblock(self, x, pfx, n_img, n):
        """AttnBlock.forward (vqgan_arch.py:636-661)."""
        c = x.shape[1]
        qkv = self._conv1x1(x, f'{pfx}.qkv', n, pro=self._gn(x, f'{pfx}.norm', n_img, n))
        # The materialised form (bmm -> softmax -> bmm) is the default: it is FASTER than the flash-style kernel at
        # every decoder shape (671 vs 845 us at N = 2048 / B = 8, 2501 vs 2981 us for two images at N = 8192,
        # profiles/r03_spatial_attention_bench.log -- both run at 80-110 TF of the exact-fp32 rate and the score
        # tensor's round trip is served by the Infinity Cache).  The flash-style kernel (no N x N tensor) takes over
        # only where the score tensor would not be reasonable to allocate (T2H_ATTN_SCORE_MB, default 2048 MB:
        # 268 MB per image at N = 8192).
        score_mb = n_img * n * n * 4 / 2**20
        if (self.flash_attn and ops.spatial_attention_ok(n, c)
                and score_mb > float(os.environ.get('T2H_ATTN_SCORE_MB', '2048'))):
            return self._conv1x1(ops.spatial_attention(qkv, n_img, n, c), f'{pfx}.proj', n, residual=x)
        q3 = qkv.view(n_img, n, 3 * c)
        s = torch.empty((n_img, n, n), device=x.device, dtype=torch.float32)
        ops.bgemm(q3[:, :, :c], q3[:, :, c:2 * c], s, alpha=float(int(c)**(-0.5)))
        ops.softmax_rows_(s)
        o = torch.empty((n_img, n, c), device=x.device, dtype=torch.float32)
        ops.bgemm(s, q3[:, :, 2 * c:], o, b_trans=True)
        return self._conv1x1(o.view(n_img * n, c), f'{pfx}.proj', n, residual=x)

    def _mid(self, h, n_img, hh, ww):
        nm = self.name
        h = self.resblock(h, f'{nm}.mid.block_1', n_img, hh, ww)
        h = self.attnblock(h, f'{nm}.mid.attn_1', n_img, hh * ww)
        return self.resblock(h, f'{nm}.mid.block_2', n_img, hh, ww)

    def _conv(self, x, pfx, n_img, h, w, mode='same', residual=None):
        """3x3 convolution without a norm in front (conv_in, Upsample / Downsample convs)."""
        if mode == 'down':
            P = self.P
            return ops.conv3x3(x, P[f'{pfx}.w'], n_img, h, w, P[f'{pfx}.w'].shape[1] // 9, bias=P[f'{pfx}.b'],
                               mode=mode, residual=residual)
        return self._norm_conv3x3(x, None, pfx, n_img, h, w, mode=mode, residual=residual)

    def encode(self, x, n_img, h, w):
        """Encoder.forward (vqgan_arch.py:892-919); x rows [n_img*h*w, Cin_pad]."""
        nm = self.name
        t = self._conv(x, f'{nm}.conv_in', n_img, h, w)
        for lv in self.desc['levels']:
            assert lv['kind'] == 'down'
            for b, blk in enumerate(lv['blocks']):
                t = self.resblock(t, f"{nm}.down.{lv['level']}.block.{b}", n_img, h, w)
                if blk['attn']:
                    t = self.attnblock(t, f"{nm}.down.{lv['level']}.attn.{b}", n_img, h * w)
            if lv['resample']:
                t = self._conv(t, f"{nm}.down.{lv['level']}.downsample", n_img, h, w, mode='down')
                h, w = h // 2, w // 2
        t = self._mid(t, n_img, h, w)
        return self._norm_conv3x3(t, f'{nm}.norm_out', f'{nm}.conv_out', n_img, h, w), h, w

    def decode(self, z, n_img, h, w, bot_h=None, upscale=False):
        """Decoder.forward (vqgan_arch.py:1000-1033).  `bot_h` is added in the
        epilogue of the level-4 Upsample conv (:1021-1024).  upscale=True feeds
        the nearest-x2 upsampled latent (fused into conv_in's operand load): the
        1024x512 interpretation of SURVEY.md 8(d), config 5."""
        nm = self.name
        t = self._conv(z, f'{nm}.conv_in', n_img, h, w, mode='up' if upscale else 'same')
        if upscale:
            h, w = 2 * h, 2 * w
        t = self._mid(t, n_img, h, w)
        levels = [lv for lv in self.desc['levels'] if lv['kind'] == 'up']
        for lv in sorted(levels, key=lambda d: -d['level']):
            for b, blk in enumerate(lv['blocks']):
                t = self.resblock(t, f"{nm}.up.{lv['level']}.block.{b}", n_img, h, w)
                if blk['attn']:
                    t = self.attnblock(t, f"{nm}.up.{lv['level']}.attn.{b}", n_img, h * w)
            if lv['resample']:
                res = bot_h if (lv['level'] == 4 and bot_h is not None) else None
                t = self._conv(t, f"{nm}.up.{lv['level']}.upsample", n_img, h, w, mode='up',
                               residual=res)
                h, w = 2 * h, 2 * w
            elif lv['level'] == 4 and bot_h is not None:
                raise _lib.T2HError('decoder level 4 has no Upsample conv to carry bot_h (vqgan_arch.py:1021-1024)')
        return self._norm_conv3x3(t, f'{nm}.norm_out', f'{nm}.conv_out', n_img, h, w), h, w

    def decode_res(self, z, n_img, h, w, upscale=False):
        """DecoderRes.forward (vqgan_arch.py:1136-1151)."""
        t = self._conv(z, f'{self.name}.conv_in', n_img, h, w, mode='up' if upscale else 'same')
        if upscale:
            h, w = 2 * h, 2 * w
        return self._mid(t, n_img, h, w)


# ---------------------------------------------------------------- transformer


class _ExactFp32:
    """One arithmetic of the sampler's layer (SamplerNet._attention_half / _tail_half spell the layer itself): which
    buffers of SamplerNet._buffers hold the operands and how the norm producer, a Linear and attention are called.
    This one: fp32 operands, the exact-fp32 kernels."""

    cfg_rows = 0  # (the split arithmetics, batch-invariant runs: see SamplerNet.invariant_rows)
    image_rows = 0  # batch-invariant runs: T, the rows of ONE image (attention runs on the form the dispatcher gives B = 1)

    def _one_image_form(self):
        """None (nothing forced), or in a batch-invariant run the attention form of a single image, asked of the
        dispatcher itself"""
        return ops.mha_split_auto_form(1, self.image_rows, self.n_head) if self.image_rows else None

    def __init__(self, net, mha=True):
        self.P, self.nm, self.n_head, self.mha = net.P, net.name, net.n_head, mha

    def buffers(self, buf):
        """(h, qk, vt, y, u): LayerNorm output, q|k|v, transposed values, attention output, GELU output"""
        return buf['h'], buf['qkv'], None, buf['y'], buf['u']

    def norm(self, i, ln, x, out, role):
        p = f'{self.nm}.{i}.{ln}'
        ops.layernorm(x, self.P[f'{p}.g'], self.P[f'{p}.b'], out=out)

    def linear(self, i, lin, a, role, m, N, K, dst, to=None, residual=None, act=ACT_NONE):
        """dst[:m] = act(a @ W(i, lin)^T + b) + residual.  role: what `a` is (h1 / y / h2 / u); to: what dst is if it
        is an operand of the next kernel (u, qk), None: fp32 rows."""
        p = f'{self.nm}.{i}.{lin}'
        ops.gemm(a, self.P[f'{p}.w'], out=dst, bias=self.P[f'{p}.b'], residual=residual, act=act)

    def qkv(self, i, h, m, C, qk, vt, T):
        self.linear(i, 'qkv', h, 'h1', m, 3 * C, C, qk)

    def attention(self, i, qk, vt, B, T, C, y):
        ops.mha_noncausal(qk, B, T, self.n_head, out=y)


class _Fp16Planes(_ExactFp32):
    """Split precision: the four Linears run on the fp16 matrix cores with 2 x fp16 planes per operand (fp32-class
    accuracy, gemm_split.hip).  The producers write split rows directly: LayerNorm -> h, attention -> y, fc1's GELU
    epilogue -> u; the residual stream x stays fp32.  mha (split_mha): attention on the fp16 matrix cores too -- the
    q|k|v projection writes q, k as split rows and v as transposed planes; without it an fp32 qkv."""
    key = 'w_split'

    def buffers(self, buf):
        return buf['h_split'], buf['qk_split'] if self.mha else buf['qkv'], buf['vt'], buf['y_split'], buf['u_split']

    def norm(self, i, ln, x, out, role):
        p = f'{self.nm}.{i}.{ln}'
        ops.layernorm_split(x, self.P[f'{p}.g'], self.P[f'{p}.b'], out)

    def linear(self, i, lin, a, role, m, N, K, dst, to=None, residual=None, act=ACT_NONE, **fmt):
        p = f'{self.nm}.{i}.{lin}'
        if self.cfg_rows:  # (without it: today's call, keyword for keyword)
            fmt = dict(fmt, cfg_rows=self.cfg_rows)
        ops.gemm_split(a, self.P[f'{p}.{self.key}'], m, N, K, out=None if to else dst, out_split=dst if to else None,
                       bias=self.P[f'{p}.b'], residual=residual, act=act, **fmt)

    def qkv(self, i, h, m, C, qk, vt, T):
        if not self.mha:
            return self.linear(i, 'qkv', h, 'h1', m, 3 * C, C, qk)
        self.linear(i, 'qkv', h, 'h1', m, 3 * C, C, qk, to='qk', vt=vt, vt_col0=2 * C, vt_T=T, vt_hd=C // self.n_head)

    def attention(self, i, qk, vt, B, T, C, y):
        if not self.mha:
            return ops.mha_noncausal_split(qk, B, T, self.n_head, y)
        with ops.mha_split_form(self._one_image_form()):
            ops.mha_split(qk, 3 * C, vt, B, T, self.n_head, out_split=y)


class _X8(_Fp16Planes):
    """x8 operands (fp16 plane + two e4m3 planes, csrc/common.h), each with the calibrated power-of-two scale of its
    (layer, role) -- activations -- or (layer, Linear) -- weights (SamplerNet.calibrate_x8)."""
    key = 'w_x8'

    def __init__(self, net):
        super().__init__(net)
        self.sw, self.sa = net._x8['w'], net._x8['a']

    def norm(self, i, ln, x, out, role):
        p = f'{self.nm}.{i}.{ln}'
        ops.layernorm_x8(x, self.P[f'{p}.g'], self.P[f'{p}.b'], out, self.sa[i, role])

    def linear(self, i, lin, a, role, *args, to=None, **kw):
        super().linear(i, lin, a, role, *args, to=to, x8=(self.sa[i, role], self.sw[i, lin]),
                       out_x8_scale=self.sa.get((i, to)), **kw)

    def attention(self, i, qk, vt, B, T, C, y):
        with ops.mha_split_form(self._one_image_form()):
            ops.mha_split_x8(qk, 3 * C, vt, B, T, self.n_head, y, self.sa[i, 'y'])


class SamplerNet:
    """TransformerMultiHead.forward (models/archs/transformer_arch.py:249-273)
    up to (not including) ln_f; ln_f + the routed head live in the sampling
    tail kernel.  24 x [LN, QKV GEMM, flash MHA, proj GEMM(+res), LN, fc1
    GEMM(+GELU), fc2 GEMM(+res)]."""

    def __init__(self, P, desc, n_head, name='tf', split=False, split_mha=True, x8=None):
        self.P, self.desc, self.n_head, self.name = P, desc, n_head, name
        self.split = split
        self._deferred = None
        # x8 (default with the split path; T2H_X8=0 opts out): the four Linears read "x8" operands -- fp16 plane +
        # two e4m3 planes (csrc/common.h) -- and run both cross terms of a K tile in ONE 8-bit matrix instruction
        # (a third fewer matrix-pipe cycles; tools/cross_term_emulation.py: the hidden state moves by 4e-5 against a
        # tolerance of 2e-4).  Needs per-tensor power-of-two scales: weights from their own maximum, activations from
        # a calibration evaluation that depends on the CHECKPOINT ALONE (calibrate_x8: fixed synthetic states, run at
        # load) -- the scales, and with them every rounding, are a function of the weights, never of what the model
        # object has been fed before.  A value beyond a scale's range raises bit 1 of the overflow word and the caller
        # re-runs THAT call on the fp16 planes (X8RangeError).
        self.x8 = bool(split and split_mha and os.environ.get('T2H_X8', '1') != '0') if x8 is None else bool(x8)
        self._x8 = None  # {'w': {(layer, lin): scale}, 'a': {(layer, role): scale}, 'act_max': ...} once calibrated
        # split_mha (with split): attention on the fp16 matrix cores too -- the q|k|v
        # projection writes q, k as split rows and v as transposed planes, no fp32 qkv
        self.split_mha = split_mha
        self._buf = {}
        self._graphs = {}       # captured sampling rounds (RoundGraph), see sample_tokens
        self.last_stats = None  # schedule.stats of the last sample_tokens run
        self.last_launch_mode = None  # 'graph' (one replay per round) / 'eager' (individual launches)
        # Batch-invariant arithmetic (per-image seeds; set by a seeded sample_tokens for its own run):
        # T > 0 = a row's bits must be those of the call on its image alone.  What depends on the batch today is only
        # WHICH kernel form a launch picks: the split GEMMs their tile configuration (by M), attention its form (by B),
        # the last layer's compacted tail the few-rows kernel or a tile (by the round's row count).  With T set the
        # Linears of the layers pick the configuration of M = T, attention the form the dispatcher gives one image, and
        # the tail always runs on the few-rows kernel, compacted or not -- as the unseeded single-image call does while
        # its rounds list at most 64 rows.
        self.invariant_rows = 0

    def _buffers(self, M, C, dev):
        key = (M, C, str(dev))
        if key not in self._buf:
            self._graphs = {}  # captured rounds hold pointers into the buffers replaced below
            e = lambda n: torch.empty((M, n), device=dev, dtype=torch.float32)
            R = self.TRIM_MAX_ROWS
            self._buf = {key: dict(x=e(C), h=e(C), qkv=e(3 * C), y=e(C), u=e(4 * C),
                                   h_split=ops.split_rows_empty(M, C, dev), y_split=ops.split_rows_empty(M, C, dev),
                                   u_split=ops.split_rows_empty(M, 4 * C, dev),
                                   qk_split=ops.split_rows_empty(M, 3 * C, dev),
                                   vt=ops.vt_empty(M // 512 if M % 512 == 0 else 1, self.n_head, 512, dev),
                                   # the last layer's tail on the changed rows (finish_tail)
                                   xc=torch.empty((R, C), device=dev, dtype=torch.float32),
                                   yc=ops.split_rows_empty(R, C, dev), hc=ops.split_rows_empty(R, C, dev),
                                   uc=ops.split_rows_empty(R, 4 * C, dev))}
        return self._buf[key]

    # The LAST layer's row-wise tail (proj + residual, LayerNorm, fc1 + GELU, fc2 + residual) only
    # matters for the rows whose logits are sampled this round -- ~16 of 4096 at B=8.  With
    # defer_tail=True, hidden() stops after the last layer's attention; finish_tail() evaluates the
    # tail on the compacted changed rows.  The Linears, the LayerNorm and the residual adds are
    # row-wise, so those rows equal the full evaluation's up to the summation order of the few-rows
    # GEMM kernel (K split over 8 waves): tolerance-level equality, not bitwise
    # (tests/test_gpu_edge_cases.py compares the tokens of both forms on the bench configuration).
    TRIM_MAX_ROWS = 256
    FEW_ROWS = 16  # a row count the split GEMM's dispatcher gives the few-rows kernel (M <= 64)

    def _arithmetic(self):
        """The arithmetic of this call (looked up per call: a caller may switch `x8` off for one run)."""
        if not self.split:
            return _ExactFp32(self)
        if self.x8 and self.split_mha:
            # (bare SamplerNets of tests / tools; the models calibrate when the checkpoint is packed.  It runs in
            # buffers of its own and may switch x8 off for a checkpoint that leaves fp16's range)
            if self.ensure_x8().x8:
                return _X8(self)
        return _Fp16Planes(self, self.split_mha)

    def _attention_half(self, ar, i, B, T, x, h, qk, vt, y, observe=None):
        """Layer i, first half: LN1 -> q|k|v Linear -> attention, on the arithmetic `ar` and its buffers (ar.buffers);
        observe(layer, role, tensor, rows, cols) sees every producer's output (calibrate_x8)."""
        M, C = B * T, self.desc['C']
        ar.norm(i, 'ln1', x, h, 'h1')
        observe and observe(i, 'h1', h, M, C)
        ar.qkv(i, h, M, C, qk, vt, T)
        ar.attention(i, qk, vt, B, T, C, y)
        observe and observe(i, 'y', y, M, C)

    def _tail_half(self, ar, i, m, x, y, h, u, observe=None):
        """proj + residual -> LN2 -> fc1 + GELU -> fc2 + residual on the first m rows of x (row-wise: the whole
        batch, or finish_tail's compacted rows)."""
        C = self.desc['C']
        ar.linear(i, 'proj', y, 'y', m, C, C, x, residual=x)
        ar.norm(i, 'ln2', x, h, 'h2')
        observe and observe(i, 'h2', h, m, C)
        ar.linear(i, 'fc1', h, 'h2', m, 4 * C, C, u, to='u', act=ACT_GELU)
        observe and observe(i, 'u', u, m, 4 * C)
        ar.linear(i, 'fc2', u, 'u', m, C, 4 * C, x, residual=x)

    def hidden(self, idx, segm_tok, tex_tok, defer_tail=False, active=None):
        """active = k < B: only the first k samples of the batch, on the first k * T rows of the SAME buffers
        (samples never interact: attention is per sample) -- the samples of a compact schedule that have no step
        left sit at the end of the batch (schedule.leave_order) and are not evaluated."""
        P, nm = self.P, self.name
        B, T = idx.shape
        C = self.desc['C']
        full = buf = self._buffers(B * T, C, idx.device)
        if self.split and self.split_mha and tuple(full['vt'].shape) != (B, self.n_head, 2, C // self.n_head, T):
            self._graphs = {}  # (captured rounds hold a pointer to the buffer replaced here)
            full['vt'] = ops.vt_empty(B, self.n_head, T, idx.device, C // self.n_head)
        if active is not None and 0 < active < B:
            k = int(active)
            buf = {name: (v[:k] if name == 'vt' else v[:k * T]) for name, v in full.items()
                   if name not in ('xc', 'yc', 'hc', 'uc')}
            idx, segm_tok, tex_tok, B = idx[:k], segm_tok[:k], tex_tok[:k], k
        x = buf['x']
        ops.embed_sum4(idx, segm_tok, tex_tok, P[f'{nm}.tok_emb'], P[f'{nm}.pos_emb'],
                       P[f'{nm}.segm_emb'], P[f'{nm}.tex_emb'], out=x)
        L = self.desc['n_layers']
        self._deferred = None
        ar = self._arithmetic()
        ar.cfg_rows = ar.image_rows = int(self.invariant_rows)
        h, qk, vt, y, u = ar.buffers(buf)
        for i in range(L):
            self._attention_half(ar, i, B, T, x, h, qk, vt, y)
            if i == L - 1 and defer_tail and self.split:
                # (the WHOLE batch's buffers: finish_tail addresses rows by their index in the batch; only
                # the first B * T rows -- the active samples -- were evaluated, and only they are listed)
                self._deferred = (full['x'], full['y_split'], B * T, C)
                return x
            self._tail_half(ar, i, B * T, x, y, h, u)
        return x

    def finish_tail(self, rows, n_rows):
        """After hidden(..., defer_tail=True): the last layer's row-wise tail.  Returns (hidden, compact):
        compact=True -> hidden[i] is row rows[i] (only the first n_rows rows of the list were evaluated)."""
        x, ys, M, C = self._deferred   # (x, ys: the whole batch's buffers; M: the rows that were evaluated)
        self._deferred = None
        buf = self._buffers(x.shape[0], C, x.device)
        if 0 < n_rows <= self.TRIM_MAX_ROWS:
            m = int(n_rows)
            xc, yc = ops.gather_rows(x, rows, m, out=buf['xc'][:m]), ops.gather_rows(ys, rows, m, out=buf['yc'][:m])
            hc, uc = buf['hc'][:m], buf['uc'][:m]
            compact = True
        else:
            m, xc, yc, compact = M, x, ys, False
            hc, uc = buf['h_split'], buf['u_split']
        ar = self._arithmetic()
        if self.invariant_rows:
            # the few-rows kernel whatever the round lists -- also when the list is too long for the compacted buffers
            # and the tail runs on all evaluated rows: the SAME image lists fewer rows in a smaller batch, and its bits
            # may not depend on which branch above its batch took (that kernel handles any M, 16 rows per workgroup)
            ar.cfg_rows = self.FEW_ROWS
        self._tail_half(ar, self.desc['n_layers'] - 1, m, xc, yc, hc, uc)
        return xc, compact

    def ensure_x8(self):
        """x8 weights packed and activation scales calibrated (once per net; a no-op on the other paths)."""
        if self.x8 and self.split and self.split_mha and self._x8 is None:
            self.calibrate_x8()
        return self

    # The calibration states: X8_CAL_SAMPLES synthetic samples over the checkpoint's own vocabulary, drawn from a
    # fixed-seed MT19937 stream (numpy's frozen legacy generator: the same numbers on every version / box).
    X8_CAL_SEED = 0x78382D63
    X8_CAL_MASKED = (1.0, 0.0, 0.5, 0.25)  # masked fraction per sample: the state every run starts from, a finished one, two in between

    def x8_calibration_states(self):
        """(idx, segm_tok, tex_tok) int64 [4, T] on the CPU -- a function of the checkpoint's SHAPES only."""
        P, nm = self.P, self.name
        T, V = P[f'{nm}.pos_emb'].shape[0], P[f'{nm}.tok_emb'].shape[0]
        n_seg, n_tex, n_class = P[f'{nm}.segm_emb'].shape[0], P[f'{nm}.tex_emb'].shape[0], P[f'{nm}.heads'].shape[1]
        rs = np.random.RandomState(self.X8_CAL_SEED)
        B = len(self.X8_CAL_MASKED)
        tex = rs.randint(0, n_tex, size=(B, T)).astype(np.int64)
        tok = np.minimum(rs.randint(0, n_class, size=(B, T)).astype(np.int64) + n_class * tex, V - 2)
        u = rs.random_sample((B, T))
        idx = np.where(u < np.asarray(self.X8_CAL_MASKED)[:, None], V - 1, tok)  # V - 1: the mask id
        seg = rs.randint(0, n_seg, size=(B, T)).astype(np.int64)
        return torch.from_numpy(idx), torch.from_numpy(seg), torch.from_numpy(tex)

    def calibrate_x8(self):
        """One-time set-up of the x8 path, at load (init-time plumbing, not on the sampling path), a function of the
        CHECKPOINT ALONE: (1) the four Linears' weights as x8 rows, each matrix with the power-of-two scale that puts
        its own maximum into [128, 256); (2) the activation scales: ONE evaluation, on the fp16-plane kernels, of four
        fixed synthetic states (x8_calibration_states) in buffers of its own; the maximum of every producer's output
        (LayerNorm 1 / 2, attention, GELU) per layer is read from the fp16 plane by t2h_split_rows_absmax and scaled
        into [16, 32) -- 14x headroom before the 8-bit planes saturate, full 4-bit precision down to 2^-10 of the
        maximum.  Nothing the model is fed later changes a scale: same (checkpoint, input, seed) -> same roundings,
        in any process, on any rank, after any history (tests/test_gpu_x8.py)."""
        P, nm, C, L = self.P, self.name, self.desc['C'], self.desc['n_layers']
        dev = P.device
        lins, roles = ('qkv', 'proj', 'fc1', 'fc2'), ('h1', 'y', 'h2', 'u')
        bits = torch.zeros(2 * 4 * L, dtype=torch.int32, device=dev)  # [weights L x 4 | activations L x 4] maxima (fp32 bits)
        slot_w = lambda i, lin: i * 4 + lins.index(lin)
        slot_a = lambda i, role: 4 * L + i * 4 + roles.index(role)
        for i in range(L):
            for lin in lins:
                ops.absmax_f32(P[f'{nm}.{i}.{lin}.w'], bits[slot_w(i, lin):])
        idx, segm_tok, tex_tok = (t.to(dev) for t in self.x8_calibration_states())
        B, T = idx.shape
        M, hd = B * T, C // self.n_head
        x = torch.empty((M, C), device=dev, dtype=torch.float32)
        hs, ys = ops.split_rows_empty(M, C, dev), ops.split_rows_empty(M, C, dev)
        us, qks = ops.split_rows_empty(M, 4 * C, dev), ops.split_rows_empty(M, 3 * C, dev)
        vt = ops.vt_empty(B, self.n_head, T, dev, hd)
        ops.split_overflow(reset=True)
        ops.embed_sum4(idx, segm_tok, tex_tok, P[f'{nm}.tok_emb'], P[f'{nm}.pos_emb'], P[f'{nm}.segm_emb'],
                       P[f'{nm}.tex_emb'], out=x)
        ar = _Fp16Planes(self)
        observe = lambda i, role, t, rows, cols: ops.split_rows_absmax(t, rows, cols, bits[slot_a(i, role):])
        for i in range(L):
            self._attention_half(ar, i, B, T, x, hs, qks, vt, ys, observe)
            self._tail_half(ar, i, M, x, ys, hs, us, observe)
        try:
            check_split_overflow('index sampler (x8 calibration)')
        except SplitOverflowError:
            # the checkpoint's activations leave fp16's range on the calibration states: no x8 scales exist for it; the
            # fp16-plane path will flag the same overflow in a run and fall back to exact fp32 (a property of the
            # checkpoint, like everything else decided here)
            import warnings
            warnings.warn('text2human_amd: x8 calibration met activations beyond fp16\'s range; this checkpoint runs '
                          'without the x8 operands')
            self.x8 = False
            return
        mx_bits = bits.cpu().numpy().view(np.float32).astype(np.float64)
        sw, sa, mx = {}, {}, {}
        for i in range(L):
            for lin in lins:
                sw[i, lin] = ops.x8_scale_for(mx_bits[slot_w(i, lin)], 256.0)
                if f'{nm}.{i}.{lin}.w_x8' not in P.t:
                    P.t[f'{nm}.{i}.{lin}.w_x8'] = ops.split_rows_x8(P[f'{nm}.{i}.{lin}.w'], sw[i, lin])
            for role in roles:
                mx[i, role] = float(mx_bits[slot_a(i, role)])
                sa[i, role] = ops.x8_scale_for(mx[i, role])
        if ops.split_overflow(reset=True):
            # (a guard, not a path: every scale is derived from its matrix's maximum, so |w| s < 256 -- and x8_scale_for
            # caps it at 2^22, without which the residual plane of a near-zero matrix (max |w| < 3.05e-5: subnormal fp16
            # plane) left the 8-bit range and this word stayed 0)
            raise _lib.T2HError('x8 weight packing overflowed')
        self._x8 = {'w': sw, 'a': sa, 'act_max': mx}

    def final_norm_and_heads(self):
        """(ln_f gamma, ln_f beta, heads [n_heads, n_class, C]): what every sampling tail reads after hidden()"""
        return tuple(self.P[f'{self.name}.{k}'] for k in ('ln_f.g', 'ln_f.b', 'heads'))

    def logits(self, idx, segm_tok, tex_tok, heads=None):
        """Full [B*T, 1024] logits per head (tests / API parity only; the
        sampling loop never materialises them)."""
        P, nm = self.P, self.name
        x = self.hidden(idx, segm_tok, tex_tok)
        xf = ops.layernorm(x, P[f'{nm}.ln_f.g'], P[f'{nm}.ln_f.b'])
        B, T = idx.shape
        out = []
        for hd in range(self.desc['n_heads']):
            if heads is not None and hd not in heads:
                out.append(None)
                continue
            out.append(ops.gemm(xf, P[f'{nm}.heads'][hd]).view(B, T, -1))
        return out


class TorchDeviceNoise:
    """Default noise source: torch's global generator of the GPU, consumed exactly like the
    reference does (rand per step; one full [B*T, 1024] exponential_ per ACTIVE head, the draw
    Categorical.sample() makes inside multinomial) so identical seeds give identical tokens.

    Normally no draw is materialised: build_schedule reproduces the `rand` draws on the device
    (t2h_unmask_schedule), the sampling tail computes the elements of the exponential_ tensors it
    needs, and the generator is advanced to where the reference's would stand.  That emulation of
    ATen's Philox kernels is verified against the installed torch at first use (`emulation_ok`);
    if it ever disagrees (another torch / ROCm build) the draws below are made for real."""

    _checked = {}

    def __init__(self, device):
        self.device = device

    def uniform(self, step, shape):
        return torch.rand(shape, device=self.device)

    def exponential(self, step, head, shape):
        return torch.empty(shape, device=self.device).exponential_(1.0)

    def generator(self):
        dev = torch.device(self.device)
        index = dev.index if dev.index is not None else torch.cuda.current_device()  # (initialises CUDA)
        return torch.cuda.default_generators[index], index

    def emulation_ok(self, n, n_class):
        """True iff t2h_philox_uniform_f32 / t2h_philox_exponential_f32 reproduce this torch build's
        `rand(n)` / `empty(n * n_class).exponential_()` bit for bit (generator state restored)."""
        gen, index = self.generator()
        key = (index, int(n), int(n_class))
        if key not in self._checked:
            state = gen.get_state()
            try:
                seed, off = gen.initial_seed(), gen.get_offset()
                want_u = torch.rand(n, device=self.device)
                off_e = gen.get_offset()
                want_e = torch.empty(n * n_class, device=self.device).exponential_(1.0)
                got_u = ops.philox_uniform(seed, off, n, self.device)
                got_e = ops.philox_exponential(seed, off_e, n * n_class, self.device)
                ok = bool(torch.equal(want_u, got_u)) and bool(torch.equal(want_e, got_e))
            finally:
                gen.set_state(state)
            if not ok:
                import warnings
                warnings.warn('text2human_amd: the in-kernel reproduction of torch\'s Philox draws does not match '
                              'this torch / ROCm build; falling back to explicit torch draws (slower, same tokens)')
            self._checked[key] = ok
        return self._checked[key]


class SplitOverflowError(_lib.T2HError):
    """An activation of the split-precision sampler left fp16's range."""


class X8RangeError(SplitOverflowError):
    """An activation of the x8 path left the range its calibrated scale gives the 8-bit planes (the fp16 planes are
    fine): the caller re-runs on the fp16-plane kernels."""


def check_split_overflow(what='sampler', knob='T2H_SPLIT_GEMM'):
    """Raises if a split-row producer flagged |x| >= 65504 since the last check (the fp16
    planes would hold inf / NaN) -- SplitOverflowError, the caller reruns with the exact-fp32 kernels -- or a value
    outside an x8 tensor's 8-bit range -- X8RangeError, the caller reruns on the fp16 planes."""
    bits = ops.split_overflow_bits(reset=True)
    if bits & 1 == 0 and bits & 2:
        raise X8RangeError(f'{what}: an activation exceeded 14x its calibration maximum, outside the range of the x8 '
                           'format\'s 8-bit planes (include/t2h_hip.h); the result is invalid.  Rerun with T2H_X8=0 '
                           '(fp16 planes).')
    if bits:
        raise SplitOverflowError(
            f'{what}: an activation reached |x| >= 65504, outside the range of the 2 x fp16 split '
            f'representation (include/t2h_hip.h); the result is invalid.  Rerun with {knob}=0 '
            '(exact-fp32 kernels).')


class SampleSchedule:
    """Device-resident schedule of one sample_tokens run (see schedule.py): rows of round r =
    rows[start[r]:start[r + 1]], each with its own noise reference."""

    def __init__(self, rows, start, round_steps, noise_kind, seed=None, offsets=None, expo_rows=None, slots=None,
                 host=None, perm=None, rng_rows=None, active=None, kept=None, seeds=None, seed_offsets=None):
        self.rows, self.start, self.round_steps = rows, start, round_steps
        # per-image seeds: seeds = one Python int per image in the SCHEDULE's sample order (the order
        # the batch has on the device; `seed` is then None), seed_offsets int64 [B] = where every image's private stream
        # ends, in the caller's order
        self.seeds, self.seed_offsets = seeds, seed_offsets
        self.kept = kept  # region editing: bool [B*T] (schedule order) of the rows that keep their source token
        self.host = host  # (row order, per-row offsets[, rng rows]) as numpy, for the padded tables of the graph path
        # finished samples leave the batch (schedule.leave_order): perm[new position] = original sample, rows /
        # round_steps are in the NEW order, rng_rows = the original row of every listed row (its noise), active[r] =
        # samples still running in round r (a prefix of the reordered batch)
        self.perm, self.rng_rows, self.active = perm, rng_rows, active
        self.noise_kind, self.seed, self.offsets, self.expo_rows, self.slots = noise_kind, seed, offsets, expo_rows, slots
        self.n_rounds = len(start) - 1
        self.max_rows = int(max(int(start[r + 1] - start[r]) for r in range(self.n_rounds))) if self.n_rounds else 0

    def row_noise(self, lo, hi):
        if self.noise_kind == 'philox':
            return ('philox', self.seed, self.offsets[lo:hi], self.rng_rows[lo:hi] if self.rng_rows is not None else None)
        return ('explicit', self.expo_rows, self.slots[lo:hi])


def _init_check(err, keep, T):
    """Region editing: the kept rows as a host bool [B*T]; raises T2HError (naming the first offending (sample, row))
    if a kept row has no source token under its texture -- t2h_edit_prefill's error word, read after the schedule's
    own host read (the stream has drained by then)."""
    e = int(err.cpu()[0])
    if e:
        r = keep.numel() - e
        raise _lib.T2HError(f'region edit: token row {r % T} of sample {r // T} is kept but its source list holds no '
                            'index under the current texture map (resample it, or give a source for that texture)')
    return keep.cpu().numpy().astype(bool)


def _texture_ids(tex_tok, n_books):
    """(tex_flat int64 [B*T] on the device, its host copy -- the schedule needs it anyway), range-checked: the reference
    raises on a bad id (transformer_arch.py:262, sample_model.py:300-317); here they would index device arrays"""
    tex_flat = tex_tok.reshape(-1).contiguous()
    tex_host = tex_flat.cpu().numpy()
    if tex_host.size and (int(tex_host.min()) < 0 or int(tex_host.max()) >= n_books):
        raise _lib.T2HError(f'texture ids must lie in [0, {n_books}), got [{int(tex_host.min())}, {int(tex_host.max())}]')
    return tex_flat, tex_host


def build_schedule(tex_tok, sample_steps, n_books, n_class, noise, compact=True, shrink=False, init=None, seeds=None):
    """The unmasking schedule + RNG bookkeeping of one sample_fn call (schedule.py), consuming
    `noise` exactly as the reference's loop would (models/sample_model.py:279-306).  shrink (compact rounds on the
    device generator only): the samples are reordered so that finished ones leave the batch (SampleSchedule.perm).
    init = (src_lists int64 [n_books, B*T], keep uint8 [B*T]) (region editing): the kept rows start unmasked and are
    never drawn; a kept row without a source token raises T2HError before the generator has moved.
    seeds (one integer in [0, 2^64) per image): every image gets the schedule, and the generator offsets,
    of the call on that image alone after manual_seed(seeds[b]) -- t2h_unmask_schedule_batch; `noise` must be the
    device generator's emulation (it is neither read nor advanced)."""
    return _schedule(*_texture_ids(tex_tok, n_books), tex_tok.shape[0], sample_steps, n_books, n_class, noise, compact,
                     shrink, init, seeds)


def _seeded_noise_check(noise, T, n_class):
    """Per-image seeds reproduce torch's draws of ONE image in the kernels: there is no explicit form of them"""
    if not isinstance(noise, TorchDeviceNoise):
        raise ValueError('seeds: per-image seeds cannot be combined with an explicit noise source')
    if not noise.emulation_ok(T, n_class):
        raise _lib.T2HError('seeds: the in-kernel reproduction of torch\'s Philox draws does not match this torch / ROCm '
                            'build, so the single-image call that defines a seeded image cannot be reproduced')


def _schedule(tex_flat, tex_host, B, sample_steps, n_books, n_class, noise, compact, shrink, init, seeds=None):
    """build_schedule on texture ids that were checked already (_texture_ids)"""
    dev, n = tex_flat.device, tex_flat.numel()
    T = n // B
    to_dev = lambda a: torch.from_numpy(a).to(dev)
    keep = err = kept = None
    if seeds is not None:
        seeds = options.image_seeds(B, seeds)
        _seeded_noise_check(noise, T, n_class)
    if init is not None:
        src_lists, keep = init
        err = ops.edit_prefill(src_lists, tex_flat, keep, 0, n_class)  # (check only: the error word)
    if seeds is not None:
        # one launch, one workgroup per image; the global generator is neither read nor advanced
        step_dev, mask_dev, rand_inc, expo_inc = ops.unmask_schedule(None, 0, tex_flat, sample_steps, n_books, n_class,
                                                                     keep=keep, seeds=seeds)
        step_of_row = step_dev.cpu().numpy()
        if init is not None:
            kept = _init_check(err, keep, T)
        head_mask = mask_dev.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        expo_off, final = schedule.draw_offsets_per_image(head_mask, sample_steps, rand_inc, expo_inc, n_books)
        p = schedule.plan_rounds(step_of_row, tex_host, B, T, compact, shrink, kept, expo_off, per_image=True)
        in_order = seeds if p.perm is None else [seeds[int(b)] for b in p.perm]
        return SampleSchedule(to_dev(p.order.astype(np.int32)), p.start, p.round_steps, 'philox', seed=None,
                              offsets=to_dev(p.offs), host=(p.order, p.offs, p.rng_rows), perm=p.perm,
                              rng_rows=to_dev(p.rng_rows), active=p.active, kept=p.kept, seeds=in_order, seed_offsets=final)
    if isinstance(noise, TorchDeviceNoise) and noise.emulation_ok(n, n_class):
        # one launch reproduces every `rand` draw; one host read fetches the whole schedule
        gen, _ = noise.generator()
        seed, off0 = gen.initial_seed(), gen.get_offset()
        step_dev, mask_dev, rand_inc, expo_inc = ops.unmask_schedule(seed, off0, tex_flat, sample_steps, n_books, n_class,
                                                                     keep=keep)
        step_of_row = step_dev.cpu().numpy()
        if init is not None:
            kept = _init_check(err, keep, T)
        head_mask = mask_dev.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        _, expo_off, final = schedule.draw_offsets(head_mask, sample_steps, off0, rand_inc, expo_inc, n_books)
        gen.set_offset(final)  # where the reference's generator stands after its loop
        p = schedule.plan_rounds(step_of_row, tex_host, B, T, compact, shrink, kept, expo_off)
        return SampleSchedule(to_dev(p.order.astype(np.int32)), p.start, p.round_steps, 'philox', seed=seed,
                              offsets=to_dev(p.offs), host=(p.order, p.offs, p.rng_rows), perm=p.perm,
                              rng_rows=None if p.rng_rows is None else to_dev(p.rng_rows), active=p.active, kept=p.kept)
    # explicit draws (tests replaying CPU noise; the emulation fallback): the reference's own loop
    # order, with the rows each head needs copied out of its full draw
    unmasked = torch.zeros(n, dtype=torch.uint8, device=dev)
    if init is not None:
        kept = _init_check(err, keep, T)  # (before the first draw)
        unmasked.copy_(keep)  # kept rows start unmasked
    changes = torch.zeros(n, dtype=torch.uint8, device=dev)
    counts = torch.zeros(n_books + 1, dtype=torch.int32, device=dev)
    rows = torch.empty(n, dtype=torch.int32, device=dev)
    step_of_row = np.zeros(n, dtype=np.int32)
    slot_of_row = np.zeros(n, dtype=np.int32)
    expo_rows = torch.empty((n, n_class), dtype=torch.float32, device=dev)
    fill = 0
    for t in range(sample_steps, 0, -1):
        rnd = noise.uniform(t, (B, T)).to(dev, torch.float32).contiguous()
        counts.zero_()
        ops.unmask_step(rnd, t, unmasked, changes, tex_flat, counts, rows, n_books)
        c = counts.cpu().numpy()
        if c[n_books] == 0:
            continue
        rows_t = np.sort(rows[:int(c[n_books])].cpu().numpy())
        step_of_row[rows_t] = t
        for h in np.nonzero(c[:n_books])[0]:  # ascending: the reference's draw order
            e = noise.exponential(t, int(h), (n, n_class)).to(dev, torch.float32).contiguous()
            rh = rows_t[tex_host[rows_t] == h]
            ops.gather_rows(e, to_dev(rh.astype(np.int32)), len(rh), out=expo_rows[fill:fill + len(rh)])
            slot_of_row[rh] = np.arange(fill, fill + len(rh), dtype=np.int32)
            fill += len(rh)
    n_kept = int(kept.sum()) if kept is not None else 0
    assert fill == n - n_kept, (fill, n, n_kept)
    p = schedule.plan_rounds(step_of_row, tex_host, B, T, compact, False, kept)
    return SampleSchedule(to_dev(p.order.astype(np.int32)), p.start, p.round_steps, 'explicit', expo_rows=expo_rows,
                          slots=to_dev(slot_of_row[p.order]), kept=kept)


def _begin_run(net, tex_tok, n_books, noise, init, temp, top_k, top_p, per_image=False):
    """What both sampling loops do first -> (noise, n_class, sp, tex_flat, tex_host); whatever raises here raises before
    the generator has moved.  sp = ops.sampling_params: the scalar temp / truncation pair, or -- any of temp / top_k /
    top_p given per image, or per_image set -- the table of the per-image tails (the caller's sample order)."""
    n_class = net.P[f'{net.name}.heads'].shape[1]
    sp = ops.sampling_params(tex_tok.shape[0], temp, top_k, top_p, n_class, per_image=per_image)
    if net.split:
        ops.split_overflow(reset=True)  # a flag left by an earlier stage is not this run's
        if net.x8:
            net.ensure_x8()  # calibration (an evaluation of its own; a no-op after a model's load) before the first round
            ops.split_overflow(reset=True)
    tex_flat, tex_host = _texture_ids(tex_tok, n_books)
    n = tex_flat.numel()
    if init is not None and (tuple(init[0].shape) != (n_books, n) or tuple(init[1].shape) != (n, )):
        raise ValueError(f'init: source lists [{n_books}, {n}] and keep [{n}] expected, got '
                         f'{tuple(init[0].shape)} / {tuple(init[1].shape)}')
    return noise or TorchDeviceNoise(tex_tok.device), n_class, sp, tex_flat, tex_host


def _initial_state(init, tex_tok, n_books, mask_id, n_class, x_t=None, out=None):
    """(x_t int64 [B, T], out int64 [n_books, B*T], err) before the first round, written into x_t / out if given: all masked
    / all -1, or with init = (src_lists, keep) in tex_tok's sample order t2h_edit_prefill's state and error word."""
    if x_t is None:
        x_t = torch.empty(tuple(tex_tok.shape), dtype=torch.int64, device=tex_tok.device)
        out = torch.empty((n_books, tex_tok.numel()), dtype=torch.int64, device=tex_tok.device)
    if init is not None:
        return x_t, out, ops.edit_prefill(init[0], tex_tok.view(-1), init[1], mask_id, n_class, x_t=x_t, out=out)
    return x_t.fill_(mask_id), out.fill_(-1), None


def _round(net, x_t, out, segm_tok, tex_tok, rows, n_rows, noise, temp, logits_ws, trunc_kw, defer=True, active=None,
           logp=None, targets=None, rank=None, seed_img=None):
    """One round of the reference's loop: the transformer on x_t (defer: the last layer's tail on the listed rows only,
    and only the first `active` samples), then the tokens of the first n_rows of `rows` drawn into x_t / out.  temp /
    trunc_kw: the scalar controls (_trunc_kw), or temp None and the per-image table (_per_image_kw).  logp (f32 [B*T],
    None = off): the drawn rows' log-probabilities (ops.sample_heads).  targets (int64 [n_books, B*T], None = off; needs
    logp): scoring -- the listed rows take their token from it instead of drawing one; rank (int32 [B*T], optional).
    seed_img (int64 [B], None = off): per-image seeds, in the order the batch has here."""
    compact = False
    if defer:
        net.hidden(x_t, segm_tok, tex_tok, defer_tail=True, active=active)
        hidden, compact = net.finish_tail(rows, n_rows)
    else:
        hidden = net.hidden(x_t, segm_tok, tex_tok)
    if logp is not None:  # (without it: today's call, keyword for keyword)
        trunc_kw = dict(trunc_kw, logp=logp)
    if targets is not None:
        trunc_kw = dict(trunc_kw, targets=targets, rank=rank)
    if seed_img is not None:
        trunc_kw = dict(trunc_kw, seed_img=seed_img, img_rows=int(tex_tok.shape[1]))
    ops.sample_heads(hidden, *net.final_norm_and_heads(), {}, rows, n_rows, tex_tok.view(-1), temp, x_t, out,
                     row_noise=noise, hidden_compact=compact, logits_ws=logits_ws, **trunc_kw)


class RoundGraph:
    """One sampling round of sample_tokens as a captured hipGraph (torch.cuda.CUDAGraph is the stream /
    graph plumbing; every node is a kernel of libt2h_hip.so).  A round is the same launch sequence with
    the same arguments every time: t2h_schedule_advance moves the round's rows / generator offsets from
    the run's padded tables into fixed staging buffers, the 24 layers and the sampling tail work on
    persistent buffers, the seed is read from device memory.  Captured once per (batch, padded rows per
    round -- a power of two --, temperature) for every count of running samples, before the first run
    (prepare), replayed for every round of every run."""

    def __init__(self, net, B, T, steps, maxr, n_books, n_class, temp, mask_id, dev, trunc=(0, 0), per_image=False,
                 logp=False, score=None, seeded=False):
        i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
        # (a weak reference: net._graphs owns this object -- a strong one would make a cycle that only the cyclic
        # collector frees, at a moment of ITS choosing, e.g. in the middle of another graph's capture)
        self._net = weakref.ref(net)
        self.maxr, self.mask_id, self.n_class = maxr, mask_id, n_class
        if per_image:
            # the table of the per-image tails: a persistent buffer the captured launches point to, filled by run()
            # before the replays like rows_tbl -- its VALUES are not captured, so they are not part of the graph key
            self.params = i32(B, 3)
            self.temp, self.trunc = None, _per_image_kw(self.params, T)
        else:
            self.params, self.temp = None, float(temp)
            self.trunc = _trunc_kw(trunc)  # (captured by value, like temp: part of the graph key)
        self.x_t, self.out, self.segm, self.tex = i64(B, T), i64(n_books, B * T), i64(B, T), i64(B, T)
        self.rows_tbl, self.offs_tbl, self.rng_tbl = i32(steps, maxr), i64(steps, maxr), i32(steps, maxr)
        self.cur_rows, self.cur_offs, self.cur_rng = i32(maxr), i64(maxr), i32(maxr)
        self.round_ctr, self.seed = i32(1), i64(1)
        # per-image seeds: a persistent buffer the captured tail points to, refreshed by run() like the per-image table
        # (the schedule's sample order) -- its VALUES are not captured: runs with other seeds replay the same graphs
        self.seed_img = i64(B) if seeded else None
        self.captures = 0  # rounds captured so far (a run that finds all its graphs adds none)
        self.logits_ws = torch.empty((maxr, n_class), dtype=torch.float32, device=dev)
        # per-token log-probabilities (return_logp): a persistent buffer the captured tail points to, NaN-filled by run()
        # beside the initial state; None = the tail without them (part of the graph key)
        self.logp = torch.empty(B * T, dtype=torch.float32, device=dev) if (logp or score) else None
        # scoring (score_tokens; `score` = the key's trailing element): the map to score, filled by run() beside the
        # initial state in the schedule's sample order, and the optional rank output (-1 = never scored)
        self.targets = i64(n_books, B * T) if score else None
        self.rank = i32(B * T) if score == SCORE_RANK else None
        self.stream = torch.cuda.Stream(device=dev)
        self.B = B
        self.graphs = {}  # samples still running (a prefix of the batch, schedule.leave_order) -> captured round
        self.pool = torch.cuda.graph_pool_handle()  # one memory pool for all of them (a capture allocates nothing big)

    def prepare(self, counts):
        """Captures the round for every count of running samples in `counts` (all of 1..B when finished samples
        leave the batch), once, before the first run: which counts a run meets depends on its seed, and a capture
        in the middle of a later run would be an eager round + a device-wide synchronisation inside the sampling
        loop.  One eager round on a valid dummy state first (it
        sizes every lazily allocated workspace); a capture itself executes nothing.  Call on self.stream."""
        _initial_state(None, self.tex, self.out.shape[0], self.mask_id, self.n_class, self.x_t, self.out)
        for t in (self.segm, self.tex, self.rows_tbl, self.offs_tbl, self.rng_tbl, self.round_ctr, self.seed,
                  self.targets, self.seed_img):
            if t is not None:
                t.zero_()
        self.body(self.B)
        self.stream.synchronize()
        for k in sorted(counts, reverse=True):
            if k not in self.graphs:
                self.capture(k)

    def body(self, k):
        """One round on the first k samples of the batch (the others have no step left)."""
        ops.schedule_advance(self.rows_tbl, self.offs_tbl, self.rng_tbl, self.round_ctr, self.cur_rows, self.cur_offs,
                             self.cur_rng, self.maxr)
        _round(self._net(), self.x_t, self.out, self.segm, self.tex, self.cur_rows, self.maxr,
               ('philox', self.seed, self.cur_offs, self.cur_rng), self.temp, self.logits_ws, self.trunc, active=k,
               logp=self.logp, targets=self.targets, rank=self.rank, seed_img=self.seed_img)

    def capture(self, k):
        g = torch.cuda.CUDAGraph()
        # thread_local: another thread of this process -- RCCL's watchdog, a data loader -- may call into
        # the HIP runtime while this thread captures.  No cyclic garbage collection inside the capture:
        # a collected tensor / graph / event would be released through the runtime in the middle of it.
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g, pool=self.pool, stream=self.stream, capture_error_mode='thread_local'):
                self.body(k)
        finally:
            if gc_was_on:
                gc.enable()
        self.graphs[k] = g
        self.captures += 1

    def run(self, sched, segm_tok, tex_tok, init=None, params=None, targets=None):
        """All rounds of one run on this graph's stream; returns `out` (valid once the caller's stream
        has waited, which this does).  init = (src_lists, keep) in the schedule's sample order (region editing):
        x_t / out start from t2h_edit_prefill instead of all-masked -- before the replays, outside any capture.
        params (a per-image graph): the run's table (ops.SAMPLE_PARAMS_DTYPE [B]) in the schedule's sample order.
        targets (a scoring graph): the map to score, int64 [n_books, B*T] in the schedule's sample order."""
        order, offs, rng_rows = sched.host
        tables = schedule.RoundTables(order, offs, sched.start, self.maxr, per_row32=rng_rows if rng_rows is not None else order)
        R, rows_tbl, offs_tbl = tables.n_rounds, tables.rows_tbl, tables.val_tbl
        active = sched.active if sched.active is not None else np.full(R, self.B, dtype=np.int64)
        caller = torch.cuda.current_stream()
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            ops.split_overflow(reset=True)  # (this stream's flag; allocated here, before any capture)
            if self.params is not None:  # (before prepare: its eager round reads a valid table)
                self.params.copy_(ops.sample_params_tensor(params, 'cpu'), non_blocking=False)
            counts = set(range(1, self.B + 1)) if sched.active is not None else {self.B}
            if not counts <= set(self.graphs):
                self.prepare(counts)
                ops.split_overflow(reset=True)
            self.rows_tbl[:R].copy_(torch.from_numpy(rows_tbl), non_blocking=False)
            self.offs_tbl[:R].copy_(torch.from_numpy(offs_tbl), non_blocking=False)
            self.rng_tbl[:R].copy_(torch.from_numpy(tables.aux32_tbl), non_blocking=False)
            self.segm.copy_(segm_tok)
            self.tex.copy_(tex_tok)
            _initial_state(init, self.tex, self.out.shape[0], self.mask_id, self.n_class, self.x_t, self.out)
            if self.logp is not None:
                self.logp.fill_(float('nan'))  # (a row that is never drawn keeps it)
            if self.targets is not None:
                self.targets.copy_(targets)
            if self.rank is not None:
                self.rank.fill_(-1)
            self.round_ctr.zero_()
            if self.seed_img is not None:
                self.seed_img.copy_(ops.seeds_tensor(sched.seeds, 'cpu'), non_blocking=False)
            else:
                self.seed.fill_(schedule.as_int64(sched.seed))  # (a uint64 seed >= 2^63 in its two's-complement form)
            for r in range(R):
                k = int(active[r])
                self.graphs[k].replay()
            check_split_overflow('index sampler')
        caller.wait_stream(self.stream)
        return self.out


def _trunc_kw(trunc):
    """validated (top_k, top_p_q) (ops.truncation_settings) -> the keyword arguments of the tail launches (p_q / 2^20 is
    exact in floating point, so the launch recovers the same p_q)"""
    k, p_q = trunc
    return dict(top_k=int(k), top_p=(int(p_q) / ops.TOP_P_ONE if p_q else 1.0))


def _per_image_kw(params, T):
    """the per-image table on the device (ops.sample_params_tensor) -> the keyword arguments of the tail launches"""
    return dict(params=params, rows_per_sample=int(T))


SCORE, SCORE_RANK = 'score', 'score+rank'  # the trailing key element of a scoring graph: without / with the rank output


def round_graph_key_per_image(B, T, sample_steps, maxr, mask_id, n_books, x8, logp=False, score=None, seeded=False):
    """The key of the captured rounds of per-image runs: the table is read from a buffer of the graph, so neither
    temperatures nor truncation settings are held by value -- runs with different values share the captures.  logp
    (the tail that also writes log-probabilities): one more trailing element, absent without it.  score (SCORE /
    SCORE_RANK: the tail that reads its tokens from a target map, score_tokens): likewise."""
    return ((B, T, sample_steps, maxr, int(mask_id), n_books, bool(x8), 'per-sample') + (('logp', ) if logp else ()) +
            ((score, ) if score else ()) + (('seeded', ) if seeded else ()))


def round_graph_key(B, T, sample_steps, maxr, temp, mask_id, n_books, x8, trunc=(0, 0), logp=False, score=None,
                    seeded=False):
    """What a captured round (RoundGraph) holds BY VALUE: two calls share a graph iff this key is equal.  logp (the tail
    that also writes log-probabilities): one more trailing element, absent without it -- the keys, and so the captures,
    of runs without it are what they always were.  score (SCORE / SCORE_RANK: the scoring tail, score_tokens): one more
    trailing element by the same rule."""
    return ((B, T, sample_steps, maxr, float(temp), int(mask_id), n_books, bool(x8), int(trunc[0]), int(trunc[1])) +
            (('logp', ) if logp else ()) + ((score, ) if score else ()) + (('seeded', ) if seeded else ()))


def sample_tokens(net, segm_tok, tex_tok, sample_steps, mask_id, temp=1.0, noise=None,
                  n_books=18, step_hook=None, round_hook=None, compact=None, init=None, top_k=None, top_p=None,
                  return_logp=False, seeds=None):
    """BaseSampleModel.sample_fn (models/sample_model.py:256-328) on device.

    The unmasking schedule and every generator offset are computed up front (build_schedule: they
    do not depend on the transformer), so the loop below never reads anything back from the GPU.
    compact=True (default; T2H_COMPACT_ROUNDS=0 or a step_hook turn it off): every sample advances
    through its own active steps -- a (sample, step) pair that changes no token is never evaluated,
    its logits would not be read (sample_model.py:300-317) -- which takes ~13.5 % fewer transformer
    evaluations than the reference's synchronous loop and gives the same tokens up to fp32 summation-order
    ties (a round's row list differs between the two schedules, and the last layer's tail picks its GEMM
    tile by the row count; on the bench configuration the tokens of both schedules are identical,
    tests/test_gpu_edge_cases.py).
    compact=False: one round per step that changes a token, all samples at that step.
    Returns int64 [18, B*T] (-1 off-texture).

    top_k / top_p: truncated sampling ("Truncated sampling"; ops.truncation_settings): every token draw is
    restricted to the classes at or above the row's threshold.  The generator is consumed as without it.

    temp / top_k / top_p may each be a sequence with one entry per image, in the caller's sample order (DESIGN.md,
    "Per-image sampling controls"; ops.sampling_params): image b is then, bit for bit, image b of the call with
    image b's values as scalars; the schedule and the generator do not depend on them.  Scalars take the scalar path.

    init = (src_lists int64 [n_books, B*T], keep uint8 [B*T]) -- region editing ("Editing a region"): the
    rows with keep != 0 start as their source token and are never resampled; everything else is the loop above, with
    the generator consumed exactly as the reference's loop started from that state would consume it.

    return_logp: returns (out, logp) -- logp float32 [B*T] in the caller's sample order, the natural-log probability of
    every drawn token under the full softmax of logits / temp at the moment it was drawn (truncation
    changes the token, never the distribution); NaN for rows that were never drawn (kept by a region edit).  Tokens and
    generator are those of the call without it.

    seeds (one integer in [0, 2^64) per image, the caller's sample order): image b is what this function
    returns for a batch that holds image b alone after torch.cuda.manual_seed(seeds[b]) -- its own schedule, its own
    generator offsets, its own noise -- whatever else is in the batch.  The global generator is neither read nor
    advanced; net.last_seed_offsets (int64 [B], numpy) = where every image's private stream ends.  Not with an explicit
    `noise` (ValueError); T2HError where the kernels cannot reproduce this torch build's draws.

    Test hooks, called after each round and allowed to overwrite x_t in place (teacher forcing):
    round_hook(r, steps, x_t, out) with steps[b] = the step sample b just took (0 = idle);
    step_hook(t, x_t, out) (compact=False only; steps that change no token are skipped)."""
    with _invariant(net, segm_tok.shape[1] if seeds is not None else 0):
        return _token_loop(net, segm_tok, tex_tok, sample_steps, mask_id, temp, noise, n_books, step_hook, round_hook,
                           compact, init, top_k, top_p, return_logp, seeds=seeds)


@contextlib.contextmanager
def _invariant(net, rows):
    """a seeded run: every launch picks its kernel form as the call on one image of `rows` token rows does
    (SamplerNet.invariant_rows); rows = 0: nothing changes"""
    net.invariant_rows = int(rows)
    try:
        yield
    finally:
        net.invariant_rows = 0


def _target_check(targets, tex_flat, n_class, T):
    """Scoring: every row's target under its own texture must be a class -- t2h_edit_prefill's check-only form with an
    all-ones keep; raises T2HError naming the first offending (sample, row), before the generator has moved."""
    ones = torch.ones(tex_flat.numel(), dtype=torch.uint8, device=tex_flat.device)
    e = int(ops.edit_prefill(targets, tex_flat, ones, 0, n_class).cpu()[0])
    if e:
        r = tex_flat.numel() - e
        raise _lib.T2HError(f'score: token row {r % T} of sample {r // T} has no index in [0, {n_class}) under the current '
                            'texture map in the token map to score')


def score_tokens(net, segm_tok, tex_tok, sample_steps, mask_id, targets, temp=1.0, noise=None, n_books=18, keep=None,
                 compact=None, round_hook=None, return_rank=False):
    """Teacher-forced per-token log-probabilities of a GIVEN token map along sample_tokens' own path.

    targets int64 [n_books, B*T] (the layout sample_tokens returns; row r's token is targets[tex[r]][r]).  The loop is
    sample_tokens' -- the same schedule, rounds, sample reordering and eager / graph decision -- except that a row's
    token is read from `targets` instead of drawn, so that the next round sees the state sampling that map would have
    produced.  Returns logp float32 [B*T] in the caller's sample order: the natural-log probability of the row's target
    under the full softmax of logits / temp at the round the schedule unmasks it; with return_rank (logp, rank), rank
    int32 [B*T] = the number of classes with a strictly greater logit (0 = the mode).

    keep (uint8 [B*T]): those rows start as their target token (init = (targets, keep)), are not scored -- NaN, rank -1
    -- and the rest is scored conditionally on them.  temp: a scalar, or one value per image.  There is no top_k /
    top_p: truncation never changed the distribution.

    Every row's own-texture target must lie in [0, n_class): T2HError (first offending (sample, row)) before the
    generator has moved.  The generator is consumed exactly as sample_tokens with the same init consumes it, the
    offsets of the exponential draws that are never made included: a map that sample_tokens(return_logp=True) drew at
    generator state G, scored at state G, returns that call's logp bits.  (Per-image seeds: score_tokens_seeded.)"""
    return _score_tokens(net, segm_tok, tex_tok, sample_steps, mask_id, targets, temp, noise, n_books, keep, compact,
                         round_hook, return_rank, None)


def score_tokens_seeded(net, segm_tok, tex_tok, sample_steps, mask_id, targets, seeds, temp=1.0, n_books=18, keep=None,
                        compact=None, return_rank=False):
    """score_tokens with per-image seeds (seeds as in sample_tokens): every image is scored along the
    schedule of its own seed, so a map drawn with sample_tokens(seeds=s, return_logp=True) scored with seeds=s returns
    that call's logp bits, whatever batch either call ran in; the global generator is not touched.  (A function of its
    own: score_tokens keeps its parameter list.)"""
    return _score_tokens(net, segm_tok, tex_tok, sample_steps, mask_id, targets, temp, None, n_books, keep, compact, None,
                         return_rank, options.image_seeds(segm_tok.shape[0], seeds))


def _score_tokens(net, segm_tok, tex_tok, sample_steps, mask_id, targets, temp, noise, n_books, keep, compact, round_hook,
                  return_rank, seeds):
    """score_tokens / score_tokens_seeded"""
    if tuple(targets.shape) != (n_books, segm_tok.numel()) or targets.dtype != torch.int64:
        raise ValueError(f'targets: int64 [{n_books}, {segm_tok.numel()}] expected, got {targets.dtype} {tuple(targets.shape)}')
    targets = targets.contiguous()
    with _invariant(net, segm_tok.shape[1] if seeds is not None else 0):
        return _token_loop(net, segm_tok, tex_tok, sample_steps, mask_id, temp, noise, n_books, None, round_hook, compact,
                           None if keep is None else (targets, keep), None, None, True,
                           score=(targets, SCORE_RANK if return_rank else SCORE), seeds=seeds)


def _token_loop(net, segm_tok, tex_tok, sample_steps, mask_id, temp, noise, n_books, step_hook, round_hook, compact, init,
                top_k, top_p, return_logp, score=None, seeds=None):
    """The loop of sample_tokens (see there).  score = (targets, SCORE or SCORE_RANK): score_tokens -- every round's
    tail reads its tokens from `targets`; returns logp, or (logp, rank)."""
    B, T = segm_tok.shape
    dev, n = segm_tok.device, B * T
    if compact is None:
        compact = step_hook is None and os.environ.get('T2H_COMPACT_ROUNDS', '1') != '0'
    if compact and step_hook is not None:
        raise ValueError('step_hook needs compact=False (samples are at different steps in a compact round)')
    if seeds is not None:  # (raises before anything is evaluated or drawn)
        seeds = options.image_seeds(B, seeds)
        if noise is not None and not isinstance(noise, TorchDeviceNoise):
            raise ValueError('seeds: per-image seeds cannot be combined with an explicit noise source')
    noise, n_class, sp, tex_flat, tex_host = _begin_run(net, tex_tok, n_books, noise, init, temp, top_k, top_p)
    table = sp.table
    targets = score_kind = None
    if score is not None:
        targets, score_kind = score
        _target_check(targets, tex_flat, n_class, T)
    # finished samples leave the batch (T2H_SHRINK_BATCH=0 opts out; hooks see the batch in its own order)
    shrink = (compact and step_hook is None and round_hook is None and os.environ.get('T2H_SHRINK_BATCH', '1') != '0')
    sched = _schedule(tex_flat, tex_host, B, sample_steps, n_books, n_class, noise, compact, shrink, init, seeds)
    net.last_seed_offsets = sched.seed_offsets
    defer = bool(net.split and net.split_mha and os.environ.get('T2H_TRIM_LAST_LAYER', '1') != '0')
    # (only the deferred-tail form of hidden() runs on the prefix of running samples; every other form evaluates the
    # whole batch each round, and the counts say so)
    net.last_stats = schedule.stats(sched.round_steps, sample_steps, sched.active if defer else None, kept=sched.kept)
    tex_tok = tex_flat.view(B, T)
    in_batch_order = lambda out: out  # [..., n] in the schedule's sample order -> the caller's
    if sched.perm is not None:
        perm_t = torch.from_numpy(sched.perm).to(dev)
        segm_tok, tex_tok = segm_tok[perm_t].contiguous(), tex_tok[perm_t].contiguous()
        if init is not None:  # the initial state in the schedule's sample order, like segm_tok / tex_tok
            init = (init[0].view(-1, B, T)[:, perm_t].reshape(-1, n).contiguous(), init[1].view(B, T)[perm_t].reshape(n))
        if targets is not None:  # the map to score, likewise
            targets = targets.view(-1, B, T)[:, perm_t].reshape(-1, n).contiguous()
        if table is not None:  # the kernels index the table by the sample's position in the batch THEY see
            table = table[sched.perm]
        caller_rows = torch.from_numpy(schedule.in_caller_order(sched.perm, B, T)).to(dev)
        in_batch_order = lambda out: out[..., caller_rows]

    # Default (T2H_GRAPH=0 opts out): every round is ONE replay of a captured launch sequence (RoundGraph)
    # instead of ~180 launches from this thread.  The GPU work is the same; what changes is the host side --
    # with one process per GPU, eight Python threads issuing ~60 k launches/s each is the scaling risk of
    # SURVEY.md 8(e).  Test hooks, explicit noise sources and the per-launch event sampling of bench.py's
    # profiling leg need individual launches and take the loop below.
    net.last_launch_mode = 'eager'
    if (os.environ.get('T2H_GRAPH', '1') != '0' and defer and sched.noise_kind == 'philox' and step_hook is None
            and round_hook is None and 0 < sched.max_rows <= net.TRIM_MAX_ROWS and ops.gemm_profile_active() is False):
        net.last_launch_mode = 'graph'
        # padded rows per round: a power of two >= 16 (at most five graph sets per batch size, whatever the seeds)
        maxr = min(net.TRIM_MAX_ROWS, max(16, 1 << (int(sched.max_rows) - 1).bit_length()))
        net._buffers(n, net.desc['C'], dev)  # (a change of batch size drops the graphs of the old buffers)
        if table is None:
            key = round_graph_key(B, T, sample_steps, maxr, temp, mask_id, n_books, net.x8, sp.trunc,
                                  logp=return_logp and score is None, score=score_kind, seeded=seeds is not None)
        else:
            key = round_graph_key_per_image(B, T, sample_steps, maxr, mask_id, n_books, net.x8,
                                            logp=return_logp and score is None, score=score_kind,
                                            seeded=seeds is not None)
        if key not in net._graphs:
            net._graphs[key] = RoundGraph(net, B, T, sample_steps, maxr, n_books, n_class, temp, mask_id, dev,
                                          trunc=sp.trunc, per_image=table is not None, logp=return_logp, score=score_kind,
                                          seeded=seeds is not None)
        graph = net._graphs[key]
        out = in_batch_order(graph.run(sched, segm_tok, tex_tok, init=init, params=table, targets=targets).clone())
        if score is not None:
            logp = in_batch_order(graph.logp.clone())
            return (logp, in_batch_order(graph.rank.clone())) if score_kind == SCORE_RANK else logp
        return (out, in_batch_order(graph.logp.clone())) if return_logp else out
    tail_kw = _trunc_kw(sp.trunc) if table is None else _per_image_kw(ops.sample_params_tensor(table, dev), T)
    x_t, out, _ = _initial_state(init, tex_tok, n_books, mask_id, n_class)
    logp = torch.full((n, ), float('nan'), dtype=torch.float32, device=dev) if return_logp else None
    rank = torch.full((n, ), -1, dtype=torch.int32, device=dev) if score_kind == SCORE_RANK else None
    logits_ws = torch.empty((max(sched.max_rows, 1), n_class), dtype=torch.float32, device=dev)
    seed_img = ops.seeds_tensor(sched.seeds, dev) if sched.seeds is not None else None
    for r in range(sched.n_rounds):
        lo, hi = int(sched.start[r]), int(sched.start[r + 1])
        k = int(sched.active[r]) if sched.active is not None else None
        _round(net, x_t, out, segm_tok, tex_tok, sched.rows[lo:hi], hi - lo, sched.row_noise(lo, hi), sp.temp, logits_ws,
               tail_kw, defer, k, logp, targets, rank, seed_img)
        if round_hook is not None:
            round_hook(r, sched.round_steps[r], x_t, out)
        if step_hook is not None:
            step_hook(int(sched.round_steps[r].max()), x_t, out)
    if net.split:
        check_split_overflow('index sampler')
    if score is not None:
        return (in_batch_order(logp), in_batch_order(rank)) if rank is not None else in_batch_order(logp)
    return (in_batch_order(out), in_batch_order(logp)) if return_logp else in_batch_order(out)


def sample_tokens_confidence(net, segm_tok, tex_tok, mask_id, rounds=16, temp=1.0, choice_temp=4.5, noise=None,
                             n_books=18, round_hook=None, init=None, top_k=None, top_p=None, return_logp=False):
    """Confidence-ordered parallel decoding ("Confidence-ordered decoding"; opt-in, sample_tokens is the
    reference's loop): `rounds` rounds, each ONE transformer evaluation of the whole batch, a token + confidence for
    every still-masked row (t2h_confidence_tail) and, per sample, the commit of the k_r rows with the largest score
    conf + tau_r * gumbel (t2h_confidence_commit).  k_r (schedule.confidence_schedule, from every sample's own number
    of masked rows), tau_r and the generator offsets of the round's two draws sit in device tables that
    t2h_schedule_advance walks, so a round is the same launch sequence with the same arguments every time and the loop
    reads nothing back.  Per round the device generator is consumed as `empty(B*T, n_class).exponential_()` then
    `rand(B*T)` would consume it (the elements needed are computed in the kernels); an explicit `noise` is asked for
    noise.exponential(r, None, (B*T, n_class)) and noise.uniform(r, (B*T, )).
    init = (src_lists, keep) as in sample_tokens.  top_k / top_p: truncated sampling as in sample_tokens -- it changes
    the token a row draws, never its confidence (the log-probability under the full softmax).  round_hook(r, x_t, out, tokens, conf, scores) is called after round
    r = 1 .. R and may overwrite x_t / out in place (teacher forcing); rounds after the last masked row of the whole
    batch are not evaluated (their draws are still counted).  Returns int64 [n_books, B*T] (-1 off-texture).
    return_logp: returns (out, logp), logp float32 [B*T] = the confidence (a log-probability already) of every committed
    row as the round that committed it formed it, NaN for rows that were never committed (kept by a region edit).

    rounds / choice_temp / temp / top_k / top_p may each be a sequence with one entry per image ("Per-image
    sampling controls"): the run has R = max rounds rounds and consumes the generator as the scalar call with R rounds;
    image b commits in rounds 1 .. rounds[b] on schedule.confidence_schedule(M0_b, rounds[b]) with tau_{b,r} =
    choice_temp[b] (1 - r / rounds[b]) and is, bit for bit, image b of the call with its values as scalars."""
    B, T = segm_tok.shape
    dev, n = segm_tok.device, B * T
    rounds_b, ct_b = options.per_image_values(B, rounds, 'rounds'), options.per_image_values(B, choice_temp, 'choice_temp')
    per_image = rounds_b is not None or ct_b is not None
    if per_image:
        rounds_b = [int(rounds)] * B if rounds_b is None else rounds_b
        ct_b = [float(choice_temp)] * B if ct_b is None else ct_b
        for b in range(B):
            if isinstance(rounds_b[b], bool) or not isinstance(rounds_b[b], numbers.Integral) or int(rounds_b[b]) < 1:
                raise ValueError(f'image {b}: rounds must be an integer >= 1, got {rounds_b[b]!r}')
            if isinstance(ct_b[b], bool) or not isinstance(ct_b[b], numbers.Real) or not float(ct_b[b]) >= 0.0:
                raise ValueError(f'image {b}: choice_temp must be >= 0, got {ct_b[b]!r}')
        R = max(int(r) for r in rounds_b)
    else:
        R = int(rounds)
        if R < 1:
            raise ValueError(f'rounds must be >= 1, got {rounds}')
        if not float(choice_temp) >= 0.0:
            raise ValueError(f'choice_temp must be >= 0, got {choice_temp}')
    noise, n_class, sp, tex_flat, _ = _begin_run(net, tex_tok, n_books, noise, init, temp, top_k, top_p, per_image)
    per_image = sp.table is not None
    if per_image and rounds_b is None:
        rounds_b, ct_b = [R] * B, [choice_temp] * B
    # (no reordering in this loop: the table is in the batch's own order)
    trunc_kw = _per_image_kw(ops.sample_params_tensor(sp.table, dev), T) if per_image else _trunc_kw(sp.trunc)
    x_t, out, err = _initial_state(init, tex_flat.view(B, T), n_books, mask_id, n_class)
    m0 = np.full(B, T, dtype=np.int64)
    if init is not None:
        kept = _init_check(err, init[1], T)  # (raises before the generator has moved)
        m0 = T - kept.reshape(B, T).sum(1).astype(np.int64)
    # the run's tables [R][w]: rows channel = k_r of every sample, 64-bit channel = generator offsets of the round's
    # exponential_ / rand draws, 32-bit channel = the bits of tau_r
    w = max(B, 2)
    if per_image:
        k_tbl, tau_tbl = schedule.confidence_tables(m0, rounds_b, ct_b, w)
    else:
        k_tbl = np.zeros((R, w), dtype=np.int32)
        for b in range(B):
            k_tbl[:, b] = schedule.confidence_schedule(int(m0[b]), R)[1]
        tau_tbl = np.zeros((R, w), dtype=np.float32)
        tau_tbl[:, 0] = schedule.confidence_choice_temps(R, choice_temp)
    off_tbl = np.zeros((R, w), dtype=np.int64)
    philox = isinstance(noise, TorchDeviceNoise) and noise.emulation_ok(n, n_class)
    seed = None
    if philox:
        gen, _ = noise.generator()
        seed, off0 = gen.initial_seed(), gen.get_offset()
        _, rand_inc = ops.torch_draw_geometry(n, dev)
        _, expo_inc = ops.torch_draw_geometry(n * n_class, dev)
        off_tbl[:, 0] = off0 + np.arange(R, dtype=np.int64) * (expo_inc + rand_inc)
        off_tbl[:, 1] = off_tbl[:, 0] + expo_inc
        gen.set_offset(off0 + R * (expo_inc + rand_inc))  # where the 2 R torch draws would leave it
    live = np.nonzero(k_tbl.sum(1))[0]
    n_eval = int(live[-1]) + 1 if live.size else 0
    net.last_stats = dict(mode='confidence', rounds=R, steps=R, batch=int(B), sample_steps_possible=int(B * R),
                          sample_steps_needed=int((k_tbl[:, :B] > 0).sum()), sample_steps_launched=int(B * n_eval),
                          rows_kept=int(n - m0.sum()))
    net.last_launch_mode = 'eager'
    k_dev, off_dev = torch.from_numpy(k_tbl).to(dev), torch.from_numpy(off_tbl).to(dev)
    tau_dev = torch.from_numpy(tau_tbl.view(np.int32)).to(dev)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    cur_k, cur_off, cur_tau = (torch.zeros(w, dtype=torch.int32, device=dev), torch.zeros(w, dtype=torch.int64, device=dev),
                               torch.zeros(w, dtype=torch.int32, device=dev))
    tok = torch.empty(n, dtype=torch.int32, device=dev)
    conf = torch.empty(n, dtype=torch.float32, device=dev)
    scores = torch.empty(n, dtype=torch.float32, device=dev)
    commit_kw = {}
    if return_logp:
        commit_kw['logp'] = logp = torch.full((n, ), float('nan'), dtype=torch.float32, device=dev)
    group_ws = ops.confidence_group_ws(n, n_books, dev)
    logits_ws = torch.empty((n, n_class), dtype=torch.float32, device=dev)
    lnf_g, lnf_b, heads = net.final_norm_and_heads()
    for r in range(1, n_eval + 1):
        ops.schedule_advance(k_dev, off_dev, tau_dev, ctr, cur_k, cur_off, cur_tau, w)
        if philox:
            noise_e, noise_u = ('philox', seed, cur_off[0:1]), ('philox', seed, cur_off[1:2])
        else:
            noise_e = ('explicit', noise.exponential(r, None, (n, n_class)).to(dev, torch.float32).contiguous())
            noise_u = ('explicit', noise.uniform(r, (n, )).to(dev, torch.float32).reshape(-1).contiguous())
        hidden = net.hidden(x_t, segm_tok, tex_tok)
        ops.confidence_tail(hidden, lnf_g, lnf_b, heads, tex_flat, x_t.view(-1), mask_id, sp.temp, noise_e, tok, conf,
                            group_ws=group_ws, logits_ws=logits_ws, **trunc_kw)
        ops.confidence_commit(conf, tok, tex_flat, noise_u, cur_k, cur_tau.view(torch.float32), mask_id, x_t, out,
                              n_class, scores=scores, per_sample=per_image, **commit_kw)
        if round_hook is not None:
            round_hook(r, x_t, out, tok, conf, scores)
    if not philox:  # the draws of the rounds that were not evaluated
        for r in range(n_eval + 1, R + 1):
            noise.exponential(r, None, (n, n_class))
            noise.uniform(r, (n, ))
    if net.split:
        check_split_overflow('index sampler')
    return (out, logp) if return_logp else out


# ---------------------------------------------------------------- UNet + heads


class UNetStack:
    """UNet.forward / ShapeUNet.forward (models/archs/unet_arch.py:470-481,
    657-674) with BN folded; returns the full-resolution decoder output
    (dec_outs[4], the only one the heads read, in_index=4)."""

    def __init__(self, P, name, desc):
        self.P, self.name, self.desc = P, name, desc

    def _cm(self, x, pfx, n_img, h, w, **kw):
        P = self.P
        cin = P[f'{pfx}.w'].shape[1] // 9
        return ops.conv3x3(x, P[f'{pfx}.w'], n_img, h, w, cin, bias=P[f'{pfx}.b'], act=ACT_RELU, **kw)

    def _attr_bias_map(self, attr, pfx, n_img, h, w):
        """Per-pixel bias of the spatially constant attribute channels: sum over
        the taps that fall inside the image of (W_attr[tap] @ attr[b])."""
        P = self.P
        wattr = P[f'{pfx}.wattr']  # [Cout, 9, A]
        cout = wattr.shape[0]
        tapc = ops.gemm(attr, wattr.view(cout * 9, -1))  # [B, Cout*9] = [B, Cout, 9]
        return ops.tap_bias_map(tapc, n_img, h, w, cout)

    def forward(self, x, n_img, h, w, attr=None):
        nm = self.name
        n_st = len(self.desc['stages'])
        skips = []
        for i in range(n_st):
            if i != 0:
                x = ops.maxpool2(x, n_img, h, w)
                h, w = h // 2, w // 2
            if attr is not None:
                bm = self._attr_bias_map(attr, f'{nm}.enc.{i}.0', n_img, h, w)
                x = self._cm(x, f'{nm}.enc.{i}.0', n_img, h, w, residual=bm, res_pre=True)
            else:
                x = self._cm(x, f'{nm}.enc.{i}.0', n_img, h, w)
            x = self._cm(x, f'{nm}.enc.{i}.1', n_img, h, w)
            skips.append((x, h, w))
        for d in reversed(range(n_st - 1)):
            skip, sh_, sw_ = skips[d]
            up = ops.bilinear_up2(x, n_img, h, w)
            h, w = 2 * h, 2 * w
            P = self.P
            cs = skip.shape[1]
            cat = torch.empty((n_img * h * w, 2 * cs), device=x.device, dtype=torch.float32)
            cat[:, :cs].copy_(skip)
            ops.gemm(up, P[f'{nm}.dec.{d}.up.w'], out=cat[:, cs:], bias=P[f'{nm}.dec.{d}.up.b'],
                     act=ACT_RELU)
            x = self._cm(cat, f'{nm}.dec.{d}.0', n_img, h, w)
            x = self._cm(x, f'{nm}.dec.{d}.1', n_img, h, w)
        return x, h, w
