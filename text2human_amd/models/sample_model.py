"""MI355X-native SampleFromParsingModel / SampleFromPoseModel.

Same public surface as the reference's models/sample_model.py (constructor
from the YAML `opt`, `feed_data`, `inference`, `sample_and_refine`,
`sample_fn`, `get_quantized_segm`, `bot_index_prediction`, the pose helpers and
the attributes callers read: .segm, .segm_tokens, .texture_mask, .device,
.batch_size, .shape, .mask_id, .sample_steps), same checkpoint files -- but
every tensor op runs in hand-written HIP kernels (libt2h_hip.so) through
text2human_amd.engine, batched over images, with no PyTorch compute fallback.
"""
import collections
import logging
import numbers
import os

import numpy as np
import torch

from .. import _lib, engine, ops, options, weights
from ..ops import ACT_RELU

logger = logging.getLogger('base')

# images decoded per pass: the decode's activations take ~0.6 GB / image at 512x256 (2.4 GB at 1024x512, where a pass
# takes a quarter of this); T2H_DECODE_CHUNK overrides (a box with less free HBM, or larger passes on an idle 288 GB)
DECODE_CHUNK = max(1, int(os.environ.get('T2H_DECODE_CHUNK', '8')))

# One refine-sampled decode: values = (temp, top_k, top_p) as validated scalars, or table = the
# per-image t2h_sample_params on the device; the noise of all `rows` = B * 512 token rows is ONE [rows, n_class]
# exponential_ draw of the generator -- philox = its (seed, offset), computed in the kernel, or expo = the tensor.
RefineDraw = collections.namedtuple('RefineDraw', 'values table philox expo rows')


class BaseSampleModel():
    """Base Model (reference: models/sample_model.py:21-340)."""

    def __init__(self, opt, state_dicts=None):
        self.opt = opt
        if not torch.cuda.is_available():
            raise RuntimeError('text2human_amd needs a ROCm GPU (MI355X); there is no CPU path')
        _lib.load()  # fail loudly if the HIP library is missing
        self.device = torch.device('cuda', torch.cuda.current_device())
        sds = state_dicts if state_dicts is not None else weights.load_checkpoints(opt)
        self._pack(sds)
        self.shape = tuple(opt['latent_shape'])
        self.mask_id = opt['codebook_size']
        self.sample_steps = opt['sample_steps']
        self.noise = None  # None -> torch's global GPU generator, like the reference
        self.batch_size = 0

    # ------------------------------------------------------------ weights
    def _pack(self, sds):
        P = weights.Params(self.device)
        self.P = P
        d_dec = weights.pack_vqgan(P, sds['decoder'], 'dec')
        d_res = weights.pack_vqgan(P, sds['bot_decoder_res'], 'res')
        d_enc = weights.pack_vqgan(P, sds['segm_encoder'], 'senc')
        # T2H_SPLIT_CONV=0 keeps the decoders' convolutions on the exact-fp32 matrix instructions;
        # default: split-precision (2 x fp16 planes, three products) like the sampler's Linears.
        # The tokenizer encoder, the index-prediction UNet and the parsing generator stay exact
        # fp32: their outputs are argmin / argmax decisions that must match the reference bit for bit.
        self.split_conv = os.environ.get('T2H_SPLIT_CONV', '1') != '0'
        if self.split_conv:
            weights.add_split_conv_weights(P, 'dec')
            weights.add_split_conv_weights(P, 'res')
        self.decoder = engine.VQGANStack(P, 'dec', d_dec)
        self.bot_decoder_res = engine.VQGANStack(P, 'res', d_res)
        self.decoder.flash_attn = self.bot_decoder_res.flash_attn = True
        self.segm_encoder = engine.VQGANStack(P, 'senc', d_enc)
        self.segm_cin_pad = P['senc.conv_in.w'].shape[1] // 9
        P.put('top.books', weights.stack_codebooks(sds['top_quantize']))
        P.put('bot.books', weights.stack_codebooks(sds['bot_quantize']))
        P.put('segm.book', sds['segm_quantizer']['embedding.weight'])
        for nm, key in (('top.pq', 'top_post_quant_conv'), ('bot.pq', 'bot_post_quant_conv'),
                        ('segm.qc', 'segm_quant_conv')):
            P.put(f'{nm}.w', weights.pack_conv1x1(sds[key]['weight']))
            P.put(f'{nm}.b', sds[key]['bias'])
        d_unet = weights.pack_unet(P, sds['guidance_encoder'], 'ipu')
        self.index_pred_guidance_encoder = engine.UNetStack(P, 'ipu', d_unet)
        self.ipd = weights.pack_multihead_fcn(P, sds['index_decoder'], 'ipd')
        d_tf = weights.pack_transformer(P, sds['sampler'], 'tf')
        self._tf_desc = d_tf
        # T2H_SPLIT_GEMM=0 selects the exact-fp32 MFMA GEMMs for the sampler's Linears;
        # default: split-precision (2 x fp16 planes, three products) on the fp16 matrix
        # cores -- same fp32-class accuracy (tests/test_gpu_split.py), higher throughput
        # (T2H_SPLIT_MHA=0 keeps the attention on the exact-fp32 kernel)
        split = os.environ.get('T2H_SPLIT_GEMM', '1') != '0'
        split_mha = os.environ.get('T2H_SPLIT_MHA', '1') != '0'
        self.sampler_fn = engine.SamplerNet(P, d_tf, self.opt['bert_n_head'], 'tf', split=split,
                                            split_mha=split_mha)
        # x8 operands (engine.SamplerNet): weights packed and the per-tensor scales of the 8-bit planes fixed HERE,
        # from the checkpoint alone -- nothing fed to the model later changes how a value is rounded
        self.sampler_fn.ensure_x8()

    # ------------------------------------------------------------ helpers
    def _texture_tokens(self, texture_mask):
        """F.interpolate(mask, (32,16), 'nearest') -> source pixel (16i,16j)
        (models/sample_model.py:187-188,264-266)."""
        b, _, hh, ww = texture_mask.shape
        sy, sx = hh // self.shape[0], ww // self.shape[1]
        return texture_mask[:, 0, ::sy, ::sx].reshape(b, -1).long().contiguous()

    # ------------------------------------------------------------ stage T
    @torch.no_grad()
    def get_quantized_segm(self, segm):
        """models/sample_model.py:330-340 -> int64 [B, 32, 16]."""
        P = self.P
        b, _, hh, ww = segm.shape
        x = ops.onehot_nhwc(segm.to(self.device, torch.float32).reshape(-1),
                            self.opt['segm_num_segm_classes'], self.segm_cin_pad)
        z, h, w = self.segm_encoder.encode(x, b, hh, ww)
        z = ops.gemm(z, P['segm.qc.w'], bias=P['segm.qc.b'])
        return ops.vq_l2_argmin(z, P['segm.book']).view(b, h, w)

    # ------------------------------------------------------------ stage S
    @torch.no_grad()
    def sample_fn(self, temp=1.0, sample_steps=None, top_k=None, top_p=None, return_logp=False, seeds=None):
        """models/sample_model.py:256-328 -> list of 18 int64 [B, 512].  top_k / top_p (not in the reference; DESIGN.md
        "Truncated sampling"): every draw only among the k most likely classes / the smallest set of most likely classes
        holding top_p of the probability.  None = off = the reference's draw.  temp / top_k / top_p may each be a
        sequence with one entry per image of the batch (DESIGN.md "Per-image sampling controls"): image b is then the
        image b of the call with its own values as scalars.  return_logp: -> (lists, logp), logp float32 [B, 512] = the
        log-probability of every drawn token under the full softmax of logits / temp when it was drawn (DESIGN.md 4.6f;
        NaN: never drawn); tokens and generator are those of the call without it.
        seeds (opt-in): one integer in [0, 2^64) per image -- image b is then what this method returns
        for a batch that holds image b alone after torch.cuda.manual_seed(seeds[b]), with the same temp / top_k / top_p /
        sample_steps: a function of (checkpoint, its own input, its own seed), not of the batch.  The global generator
        is neither read nor advanced; self.last_seed_offsets (int64 [B]) = the generator offset each of those
        single-image calls would end at."""
        return self._sample(temp, sample_steps or self.sample_steps, top_k=top_k, top_p=top_p, return_logp=return_logp,
                            seeds=seeds)

    @torch.no_grad()
    def sample_fn_confidence(self, rounds=16, temp=1.0, choice_temp=4.5, top_k=None, top_p=None, return_logp=False,
                             seeds=None):
        """Confidence-ordered parallel decoding (opt-in; DESIGN.md "Confidence-ordered decoding"): all tokens in
        `rounds` transformer evaluations instead of one per active step -> list of 18 int64 [B, 512] like sample_fn.
        rounds / choice_temp / temp / top_k / top_p may each be a sequence with one entry per image.  return_logp: as in
        sample_fn (the confidence of every committed token, from the round that committed it).  seeds: not supported on
        this path yet (ValueError, nothing drawn)."""
        self._no_seeds(seeds, 'sample_fn_confidence')
        return self._sample(temp, None, confidence=self._confidence_args(rounds, choice_temp), top_k=top_k, top_p=top_p,
                            return_logp=return_logp)

    @staticmethod
    def _confidence_args(rounds, choice_temp):
        """(rounds, choice_temp) for _sample: scalars as int / float, per-image sequences as they are"""
        return (rounds if options.is_per_image(rounds) else int(rounds),
                choice_temp if options.is_per_image(choice_temp) else float(choice_temp))

    def _confidence_options(self):
        """(rounds, choice_temp) if the options select `sample_order: confidence`, else None (the reference's loop)."""
        return options.sampling_order(self.opt)

    def _truncation_options(self):
        """(top_k, top_p) of the options `sample_top_k` / `sample_top_p` (None, None: off)."""
        return options.sampling_truncation(self.opt)

    @staticmethod
    def _no_seeds(seeds, what):
        """the paths whose draws still come from the shared generator stream refuse per-image seeds"""
        if seeds is not None:
            raise ValueError(f'{what}: per-image seeds are not supported on this path (its draws use the shared generator '
                             'stream); use sample_fn / resample_fn(order=\'random\') / score_fn')

    def _sample(self, temp, sample_steps, init=None, confidence=None, top_k=None, top_p=None, return_logp=False,
                score=None, seeds=None):
        """sample_fn's body (init: engine.sample_tokens' initial state of a region edit; confidence = (rounds,
        choice_temp): engine.sample_tokens_confidence instead of the reference's loop; top_k / top_p: truncated
        sampling, passed to every attempt of the fall-back chain below; return_logp: -> (lists, logp [B, 512]), the
        log-probabilities of the attempt that produced the tokens; score = (targets [18, B*512], keep or None,
        return_rank): engine.score_tokens on that map instead of a draw -> logp [B, 512], or (logp, rank)).  seeds: per-image
        seeds of sample_tokens / score_tokens; every attempt of the fall-back chain runs with the same ones."""
        logp_kw = dict(return_logp=True) if return_logp else {}  # (without it: today's calls, keyword for keyword)
        seed_kw = {}
        if seeds is not None:
            seed_kw = dict(seeds=options.image_seeds(self.batch_size, seeds))  # (raises before anything is drawn)
            if self.noise is not None and not isinstance(self.noise, engine.TorchDeviceNoise):
                raise ValueError('seeds: per-image seeds cannot be combined with an explicit noise source')
        ops.sampling_params(self.batch_size, temp, top_k, top_p)  # (raises before anything is evaluated or drawn)
        tex_tok = self._texture_tokens(self.texture_mask)
        # The reference computes ANY checkpoint in fp32 (transformer_arch.py:91-99).  The split-precision kernels
        # cover |x| < 65504; an activation outside raises SplitOverflowError at the end of the run -- after
        # build_schedule has advanced the generator.  So: remember the generator, and on overflow restore it and
        # run THIS call on the exact-fp32 kernels (same schedule, same draws, the reference's tokens).
        gen = torch.cuda.default_generators[self.device.index]
        state = gen.get_state()
        net = self.sampler_fn
        x8_was = net.x8
        try:
            for _ in range(3):  # x8 planes -> fp16 planes -> exact fp32, each at most once
                try:
                    if score is not None and seeds is not None:
                        out = engine.score_tokens_seeded(net, self.segm_tokens.contiguous(), tex_tok, sample_steps,
                                                         self.mask_id, score[0], seed_kw['seeds'], temp=temp, keep=score[1],
                                                         return_rank=score[2])
                    elif score is not None:
                        out = engine.score_tokens(net, self.segm_tokens.contiguous(), tex_tok, sample_steps, self.mask_id,
                                                  score[0], temp=temp, noise=self.noise, keep=score[1],
                                                  return_rank=score[2])
                    elif confidence is not None:
                        out = engine.sample_tokens_confidence(net, self.segm_tokens.contiguous(), tex_tok, self.mask_id,
                                                              rounds=confidence[0], temp=temp,
                                                              choice_temp=confidence[1], noise=self.noise, init=init,
                                                              top_k=top_k, top_p=top_p, **logp_kw)
                    else:
                        out = engine.sample_tokens(net, self.segm_tokens.contiguous(), tex_tok, sample_steps,
                                                   self.mask_id, temp=temp, noise=self.noise, init=init,
                                                   top_k=top_k, top_p=top_p, **logp_kw, **seed_kw)
                    break
                except engine.X8RangeError as e:
                    # an activation beyond 14x its calibration maximum: the 8-bit planes saturated, the fp16 planes are
                    # fine -- THIS call is re-run on the fp16-plane kernels (about 15 % slower) from the same generator
                    # state; the next call starts on x8 again (the result of a call never depends on an earlier one)
                    if not _overflow_fallback('index sampler (x8 range)', 'T2H_X8', e, 'fp16-plane'):
                        raise
                    net.x8 = False
                    gen.set_state(state)
                except engine.SplitOverflowError as e:
                    if net is not self.sampler_fn or not _overflow_fallback('index sampler', 'T2H_SPLIT_GEMM', e):
                        raise
                    gen.set_state(state)
                    net = self._exact_sampler()
        finally:
            self.sampler_fn.x8 = x8_was
        offs = getattr(net, 'last_seed_offsets', None) if seeds is not None else None
        self.last_seed_offsets = None if offs is None else torch.from_numpy(np.asarray(offs, dtype=np.int64).copy())
        b = self.batch_size
        if score is not None:
            return (out[0].view(b, -1), out[1].view(b, -1)) if score[2] else out.view(b, -1)
        if return_logp:
            out, logp = out
            return [out[i].view(b, -1) for i in range(out.shape[0])], logp.view(b, -1)
        return [out[i].view(b, -1) for i in range(out.shape[0])]

    @torch.no_grad()
    def sample_best_of(self, n, order=None, **sampling_kwargs):
        """Best-of-N by likelihood (opt-in): runs the selected sampler n times in a row on the fed batch
        -- candidate c is, bit for bit, the c-th consecutive plain call from the same generator state, and the generator
        ends where n calls leave it -- and keeps, per image, the candidate with the highest mean log-probability per
        drawn token (t2h_logp_summary: sum / count; no drawn token: -inf; ties go to the earlier candidate).
        order: 'random' (sample_fn), 'confidence' (sample_fn_confidence) or None = what the options select;
        sampling_kwargs go to that method unchanged (per-image controls included).  -> (lists, logp, score, choice):
        18 x int64 [B, 512] and float32 [B, 512] of the kept candidates, score float32 [B], choice int64 [B].  n = 1 is
        the plain call.  The selection runs on the device; nothing is read back."""
        n = options.best_of_value(n)
        self._no_seeds(sampling_kwargs.get('seeds'), 'sample_best_of')
        if order is None:
            order = 'confidence' if self._confidence_options() is not None else 'random'
            if order == 'confidence' and 'rounds' not in sampling_kwargs and 'choice_temp' not in sampling_kwargs:
                sampling_kwargs = dict(sampling_kwargs)
                sampling_kwargs['rounds'], sampling_kwargs['choice_temp'] = self._confidence_options()
        if order not in options.SAMPLE_ORDERS:
            raise ValueError(f'order must be one of {options.SAMPLE_ORDERS}, got {order!r}')
        sampler = self.sample_fn_confidence if order == 'confidence' else self.sample_fn
        b, t_len = self.batch_size, self.shape[0] * self.shape[1]
        best = best_logp = best_score = choice = None
        for c in range(n):
            lists, logp = sampler(return_logp=True, **sampling_kwargs)
            logp = logp.contiguous()
            s, cnt, _ = ops.logp_summary(logp)
            score = torch.where(cnt > 0, s / cnt.to(torch.float32), torch.full_like(s, float('-inf')))
            cand = torch.stack([x.reshape(-1) for x in lists]).contiguous()  # [18, B*512]
            if c == 0:
                best, best_logp, best_score = cand, logp, score
                choice = torch.zeros(b, dtype=torch.int64, device=self.device)
                continue
            better = score > best_score  # (strictly: a tie keeps the earlier candidate)
            rows = better.to(torch.uint8).repeat_interleave(t_len).contiguous()
            ops.merge_kept_indices(cand, rows, best)  # best[:, r] = cand[:, r] for the rows of the images that improved
            best_logp = torch.where(better[:, None], logp, best_logp)
            best_score = torch.where(better, score, best_score)
            choice = torch.where(better, torch.full_like(choice, c), choice)
        return [best[i].view(b, -1) for i in range(best.shape[0])], best_logp, best_score, choice

    # ------------------------------------------------------------ region editing
    # DESIGN.md "Editing a region": the reference loop started from a partially known state.  A token row is kept
    # (keep = 1) or resampled (keep = 0); kept rows start as their source token and are never drawn, everything else
    # is sample_fn unchanged -- with keep all zero, resample_fn IS sample_fn (same tokens, same generator offset).
    def _token_lists(self, lists, what):
        """18 x [B, 512] (or [18, B*512]) int64 -> contiguous [18, B*512] on the device."""
        n = self.batch_size * self.shape[0] * self.shape[1]
        t = lists if torch.is_tensor(lists) else torch.stack([x.reshape(-1) for x in lists])
        if t.numel() != 18 * n:
            raise ValueError(f'{what}: 18 index lists of {n} tokens expected, got {tuple(t.shape)}')
        return t.reshape(18, n).to(self.device, torch.int64).contiguous()

    def _keep_rows(self, keep):
        n_tok = self.shape[0] * self.shape[1]
        if tuple(keep.shape) != (self.batch_size, n_tok):
            raise ValueError(f'keep must be [{self.batch_size}, {n_tok}], got {tuple(keep.shape)}')
        return keep.to(self.device, torch.uint8).reshape(-1).contiguous()

    @torch.no_grad()
    def region_keep(self, region=None, labels=None):
        """-> uint8 [B, 512]: 1 for the token rows an edit keeps, 0 for the rows it resamples.  A row is resampled iff
        ANY pixel of its H/32 x W/16 cell lies in the region: `region` [B, 1, H, W] (uint8 / bool / float, nonzero =
        edit) or `labels` (parsing label ids, resolved against the current self.segm)."""
        if (region is None) == (labels is None):
            raise ValueError('region_keep: give exactly one of region (a pixel mask) or labels (parsing label ids)')
        th, tw = self.shape
        if region is not None:
            b, hh, ww = self.batch_size, self.texture_mask.shape[2], self.texture_mask.shape[3]
            if tuple(region.shape) != (b, 1, hh, ww):
                raise ValueError(f'region must be [{b}, 1, {hh}, {ww}] like the texture map, got {tuple(region.shape)}')
            m = region.to(self.device)
            if m.dtype not in (torch.uint8, torch.bool, torch.float32):
                m = m.to(torch.float32)
            return ops.region_keep(b, hh, ww, (th, tw), mask=m.contiguous())
        segm = self.segm.to(self.device, torch.float32).contiguous()  # (the dtype the tokenizer reads)
        b, _, hh, ww = segm.shape
        return ops.region_keep(b, hh, ww, (th, tw), parsing=segm, labels=[int(x) for x in labels])

    @torch.no_grad()
    def resample_fn(self, top_indices_list, keep, temp=1.0, sample_steps=None, order='random', rounds=None,
                    choice_temp=4.5, top_k=None, top_p=None, return_logp=False, seeds=None):
        """sample_fn started from `top_indices_list` (18 x int64 [B, 512], e.g. an earlier sample_fn result or a photo's
        top_encode indices) with the rows where keep [B, 512] is nonzero kept.  -> list of 18 int64 [B, 512] in
        sample_fn's format.  A kept row must have an index under the CURRENT texture map (T2HError otherwise; nothing
        changes).  order='confidence': the masked rows are filled by confidence-ordered decoding in `rounds` (default
        16) rounds, every sample on the schedule of its own number of resampled rows.  top_k / top_p: truncated
        sampling of the resampled rows, as in sample_fn.  temp / top_k / top_p / rounds / choice_temp may each be a
        sequence with one entry per image, as in sample_fn / sample_fn_confidence.  return_logp: -> (lists, logp) as in
        sample_fn; the kept rows are NaN.  seeds (order='random' only; as in sample_fn): image b is the single-image
        resample_fn call on image b after manual_seed(seeds[b])."""
        if order not in ('random', 'confidence'):
            raise ValueError(f"order must be 'random' or 'confidence', got {order!r}")
        if order == 'confidence':
            self._no_seeds(seeds, "resample_fn(order='confidence')")
        init = (self._token_lists(top_indices_list, 'resample_fn'), self._keep_rows(keep))
        if not options.is_per_image(rounds):
            rounds = int(rounds or 16)
        confidence = self._confidence_args(rounds, choice_temp) if order == 'confidence' else None
        return self._sample(temp, sample_steps or self.sample_steps, init=init, confidence=confidence, top_k=top_k,
                            top_p=top_p, return_logp=return_logp, seeds=seeds)

    @torch.no_grad()
    def score_fn(self, top_indices_list, keep=None, temp=1.0, sample_steps=None, return_rank=False, summary=False):
        """Teacher-forced per-token log-probabilities of a GIVEN token map (opt-in): how likely the
        sampler holds `top_indices_list` (18 x int64 [B, 512] or [18, B*512], as resample_fn / decode_indices accept:
        an earlier result, an edit, a candidate, a photo's top_encode indices) along sample_fn's own path -- the same
        schedule from the current generator state, every row's token read from the map instead of drawn.  -> logp
        float32 [B, 512]: the log-probability of the row's token under the full softmax of logits / temp at the round
        that unmasks it.  A map that sample_fn(return_logp=True) drew at generator state G, scored at state G with the
        same temp / sample_steps, returns that call's logp bits; the generator ends where sample_fn leaves it.
        keep [B, 512] (as in resample_fn; region_keep's output): those rows are given, not scored (NaN, rank -1); the
        rest is scored conditionally on them, as resample_fn draws them.  temp: a scalar or one value per image.
        return_rank: also rank int32 [B, 512] = the number of classes the model held strictly more likely (0 = its
        mode).  summary: also the per-image (sum, count, min) of the scored rows (t2h_logp_summary).  Returns logp, or
        the tuple (logp[, rank][, (sum, count, min)]).  Every row's token under the current texture map must be a class
        index: T2HError naming the first offending (sample, row), nothing drawn.  (Per-image seeds: score_fn_seeded.)"""
        return self._score(top_indices_list, keep, temp, sample_steps, return_rank, summary, None)

    @torch.no_grad()
    def score_fn_seeded(self, top_indices_list, seeds, keep=None, temp=1.0, sample_steps=None, return_rank=False,
                        summary=False):
        """score_fn with per-image seeds (opt-in; seeds as in sample_fn): every image is scored along the
        schedule of its own seed -- a map drawn by sample_fn(seeds=s, return_logp=True) scored with seeds=s returns that
        call's logp bits, whatever batch either call ran in; the global generator is not touched.  Everything else is
        score_fn.  (A method of its own: score_fn keeps its parameter list.)"""
        return self._score(top_indices_list, keep, temp, sample_steps, return_rank, summary,
                           options.image_seeds(self.batch_size, seeds))

    def _score(self, top_indices_list, keep, temp, sample_steps, return_rank, summary, seeds):
        """score_fn / score_fn_seeded"""
        # (everything below raises before anything is evaluated or drawn)
        self._score_temp(temp, 'score_fn')
        targets = self._token_lists(top_indices_list, 'score_fn')
        keep = None if keep is None else self._keep_rows(keep)
        out = self._sample(temp, sample_steps or self.sample_steps, score=(targets, keep, bool(return_rank)), seeds=seeds)
        res = list(out) if return_rank else [out]
        if summary:
            res.append(ops.logp_summary(res[0].contiguous()))
        return res[0] if len(res) == 1 else tuple(res)

    # ------------------------------------------------------------ self-correction
    # the sampler's own transformer as an order-free critic (pll_fn: K evaluations on a fold lattice),
    # and the loop that re-masks the rows it likes least, redraws them and keeps what it prefers (revise_fn).
    @torch.no_grad()
    def pll_fn(self, top_indices_list, keep=None, folds=4, temp=1.0, return_rank=False, summary=False):
        """Pseudo-log-likelihood of a GIVEN token map (opt-in): -> pll float32 [B, 512], for every row
        the log-probability of its token under the full softmax of logits / temp when the transformer sees the map with
        the non-kept rows of the row's FOLD replaced by the mask token and every other row as given -- on the rows of
        fold k what score_fn(map, keep=keep_k[k], temp=temp, sample_steps=1) computes.  folds (2, 4, 8 or 16) = the
        number of transformer evaluations; the lattice is t2h_fold_keep's (for folds >= 4 a hidden row sees all eight
        neighbours).  Input formats, keep, temp (a scalar or one value per image), return_rank and summary as in
        score_fn; the rows in keep are NaN / rank -1; a token without an index under the current texture map raises
        T2HError and nothing is evaluated.  Nothing is drawn: the generator is neither read nor advanced, two calls
        return the same bits, and an image's numbers do not depend on the batch it is scored in (the arithmetic of
        per-image seeds)."""
        folds = options.revise_folds_value(folds)
        self._score_temp(temp, 'pll_fn')
        targets = self._token_lists(top_indices_list, 'pll_fn')
        keep = None if keep is None else self._keep_rows(keep)
        pll, rank = self._pll(targets, keep, folds, temp, bool(return_rank))
        b = self.batch_size
        res = [pll.view(b, -1)] + ([rank.view(b, -1)] if return_rank else [])
        if summary:
            res.append(ops.logp_summary(res[0]))
        return res[0] if len(res) == 1 else tuple(res)

    def _score_temp(self, temp, what):
        """the temperature of a scoring call, validated: a finite number > 0, or one per image"""
        if not options.is_per_image(temp) and (isinstance(temp, bool) or not isinstance(temp, numbers.Real) or
                                               not 0.0 < float(temp) < float('inf')):
            raise ValueError(f'{what}: temp must be a finite number > 0, got {temp!r}')
        ops.sampling_params(self.batch_size, temp)  # (a per-image sequence: its length and every entry)

    def _critic_net(self):
        """The sampler's transformer with buffers and captured rounds of its own (built on first use; shares weights and
        x8 scales): the critic's batch of K * B images does not replace the buffers sample_fn's captured rounds point to."""
        s = self.sampler_fn
        if getattr(self, '_critic', None) is None or self._critic_of is not s:
            c = engine.SamplerNet(self.P, self._tf_desc, self.opt['bert_n_head'], 'tf', split=s.split,
                                  split_mha=s.split_mha, x8=s.x8)
            c._x8 = s.ensure_x8()._x8
            c.x8 = s.x8  # (a calibration that left fp16's range switched it off)
            self._critic, self._critic_of = c, s
        return self._critic

    def _pll(self, targets, keep, folds, temp, want_rank=False):
        """pll_fn on targets int64 [18, B*512] / keep uint8 [B*512] or None -> (pll f32 [B*512], rank int32 or None).
        The K evaluations are score_tokens_seeded runs of ONE step (every non-kept row is unmasked -- scored -- by the
        single round, whatever the seed): through _sample, so its fall-back chain applies; the seeded form neither reads
        nor advances the generator and computes every image as the call on it alone would."""
        b, t_len, cells = self.batch_size, self.shape[0] * self.shape[1], tuple(self.shape)
        n = b * t_len
        tex_flat = self._texture_tokens(self.texture_mask).reshape(-1)
        n_class = self.P['tf.heads'].shape[1]
        engine._target_check(targets, tex_flat, n_class, t_len)  # (names the caller's (sample, row); nothing evaluated)
        keep_k = ops.fold_keep(folds, b, cells, keep, device=self.device)
        logp_k = torch.empty((folds, n), dtype=torch.float32, device=self.device)
        rank_k = torch.empty((folds, n), dtype=torch.int32, device=self.device) if want_rank else None
        saved = (self.batch_size, self.segm_tokens, self.texture_mask, self.noise, self.sampler_fn,
                 getattr(self, 'last_seed_offsets', None))
        try:
            self.noise = None  # (nothing is drawn: an explicit noise source has no say here)
            if options.pll_batched(b, folds):
                # one batch of K * B images: image k * B + j = image j with fold k hidden
                self.batch_size = folds * b
                self.segm_tokens = self.segm_tokens.repeat(folds, 1)
                self.texture_mask = self.texture_mask.repeat(folds, 1, 1, 1)
                self.sampler_fn = self._critic_net()
                t_kb = targets.view(-1, 1, n).expand(-1, folds, n).reshape(targets.shape[0], folds * n).contiguous()
                temp_kb = list(options.per_image_values(b, temp, 'temp')) * folds if options.is_per_image(temp) else temp
                out = self._sample(temp_kb, 1, score=(t_kb, keep_k.view(-1), want_rank), seeds=[0] * (folds * b))
                logp_k = (out[0] if want_rank else out).reshape(folds, n).contiguous()
                rank_k = out[1].reshape(folds, n).contiguous() if want_rank else None
            else:
                for k in range(folds):
                    out = self._sample(temp, 1, score=(targets, keep_k[k].view(-1), want_rank), seeds=[0] * b)
                    logp_k[k].copy_((out[0] if want_rank else out).reshape(-1))
                    if want_rank:
                        rank_k[k].copy_(out[1].reshape(-1))
        finally:
            (self.batch_size, self.segm_tokens, self.texture_mask, self.noise, self.sampler_fn,
             self.last_seed_offsets) = saved
        out = ops.fold_gather(logp_k, folds, b, cells, rank_k=rank_k)
        return out if want_rank else (out, None)

    _FRACTION_DEFAULT = float(options.REVISE_FRACTION)  # (the default OBJECT: tells "not given" from a given 0.25)

    @torch.no_grad()
    def revise_fn(self, top_indices_list, passes=1, fraction=_FRACTION_DEFAULT, count=None, keep=None, folds=4,
                  accept='improve', temp=1.0, critic_temp=1.0, sample_steps=None, order='random', rounds=None,
                  choice_temp=4.5, top_k=None, top_p=None, seeds=None, return_trace=False):
        """Self-correction of a GIVEN token map (opt-in) -> 18 x int64 [B, 512] in sample_fn's format,
        with return_trace (lists, trace).  Every pass: the m_b rows of image b with the lowest pll_fn(map, keep, folds,
        critic_temp) are re-masked (t2h_select_lowest) and redrawn given everything else (resample_fn with temp /
        sample_steps / order / rounds / choice_temp / top_k / top_p), the candidate is scored by the same critic, and --
        accept='improve' -- image b takes it iff the t2h_logp_summary sum of its pll is STRICTLY greater (accept='always':
        every image takes it).  m_b = min(count, eligible_b) with count (an integer or one per image), else
        max(1, floor(fraction * eligible_b + 0.5)), eligible_b = the rows of image b not in keep (0 rows: nothing is
        redone; if that holds for every image the pass makes no resample_fn call); fraction in (0, 1], a scalar or one
        per image; giving both is a ValueError.  keep [B, 512]: rows that are given -- never scored, selected or redrawn.
        seeds (order='random' only): pass p redraws image b with (seeds[b] + p) mod 2^64, as resample_fn does; the
        global generator does not move.  Without seeds it moves exactly as the resample_fn calls move it.
        trace: one dict per pass -- selected uint8 [B, 512] (1 = redrawn), sum_before / sum_after f32 [B], accepted
        bool [B].  With accept='improve' the summary sum of pll_fn(result, keep, folds, critic_temp) is >= that of
        pll_fn(input, ...) for every image.  What the critic prefers is the model's own judgement, nothing more: no
        claim about image quality is made."""
        # (everything below raises before anything is evaluated or drawn)
        passes = options.revise_passes_value(passes)
        folds = options.revise_folds_value(folds)
        always = options.revise_accept_value(accept) == 'always'
        if count is not None and fraction is not self._FRACTION_DEFAULT:
            raise ValueError('revise_fn: give either fraction or count, not both')
        self._score_temp(critic_temp, 'revise_fn (critic_temp)')
        if order not in ('random', 'confidence'):
            raise ValueError(f"order must be 'random' or 'confidence', got {order!r}")
        if order == 'confidence':
            self._no_seeds(seeds, "revise_fn(order='confidence')")
        if seeds is not None:
            seeds = options.image_seeds(self.batch_size, seeds)
        ops.sampling_params(self.batch_size, temp, top_k, top_p)
        b, t_len = self.batch_size, self.shape[0] * self.shape[1]
        keep_rows = None if keep is None else self._keep_rows(keep)
        eligible = [t_len] * b if keep_rows is None else [t_len - int(x) for x in
                                                          (keep_rows.view(b, t_len) != 0).sum(1).tolist()]
        m = options.revise_row_counts(eligible, None if count is not None else fraction, count)
        cur = self._token_lists(top_indices_list, 'revise_fn').clone()
        m_dev = torch.tensor(m, dtype=torch.int32).to(self.device)
        cur_pll = self._pll(cur, keep_rows, folds, critic_temp)[0]
        cur_sum = ops.logp_summary(cur_pll, b, t_len)[0]
        steps = []  # per pass: (sel_keep or None, sum_before, sum_after, accepted uint8 or None)
        for p in range(passes):
            if not any(m):
                steps.append((None, cur_sum, cur_sum, None))
                continue
            # (from the candidate's scoring to this selection: kernels of the library only, nothing read back)
            sel_keep, _ = ops.select_lowest(cur_pll.view(b, t_len), m_dev)
            seed_kw = {} if seeds is None else dict(seeds=[(s + p) % (1 << 64) for s in seeds])
            cand = self._token_lists(self.resample_fn(cur, sel_keep, temp=temp, sample_steps=sample_steps, order=order,
                                                      rounds=rounds, choice_temp=choice_temp, top_k=top_k, top_p=top_p,
                                                      **seed_kw), 'revise_fn')
            cand_pll = self._pll(cand, keep_rows, folds, critic_temp)[0]
            cand_sum = ops.logp_summary(cand_pll, b, t_len)[0]
            new_sum, accepted = ops.accept_merge(cand, cand_pll, cand_sum, cur, cur_pll, cur_sum, b, always=always)
            steps.append((sel_keep, cur_sum, cand_sum, accepted))
            cur_sum = new_sum
        lists = [cur[i].view(b, -1) for i in range(cur.shape[0])]
        if not return_trace:
            return lists
        trace = []
        for sel_keep, before, after, accepted in steps:
            if sel_keep is None:
                selected = torch.zeros((b, t_len), dtype=torch.uint8, device=self.device)
                accepted = torch.full((b, ), always, dtype=torch.bool, device=self.device)
            else:
                selected, accepted = 1 - sel_keep, accepted != 0
            trace.append(dict(selected=selected, sum_before=before, sum_after=after, accepted=accepted))
        return lists, trace

    @torch.no_grad()
    def edit_and_refine(self, top_indices_list, region=None, labels=None, bot_indices_list=None, save_dir=None,
                        img_name=None, order='random', rounds=None, choice_temp=4.5, top_k=None, top_p=None, temp=1.0,
                        refine_temp=None, refine_top_k=None, refine_top_p=None, source_image=None, blend_hi=4,
                        blend_lo=32):
        """Region edit end to end: resample the top tokens of the region (region_keep), predict the bottom indices,
        keep `bot_indices_list` (e.g. a photo's bot_encode) outside the region if given, decode.  Return values and
        files follow sample_and_refine: with save_dir and img_name both None the first image f32 [1, 3, H, W];
        otherwise {save_dir}/{img_name[i]} PNGs are written and their uint8 [B, H, W, 3] pixels returned.  The edited
        index lists are left in self.edit_top_indices_list / self.edit_bot_indices_list (18 x int64 [B, 512]).
        refine_temp / refine_top_k / refine_top_p: the bottom indices are drawn (decode_indices); kept tokens keep
        theirs whatever these are.  source_image: the photo the index lists were encoded from, f32
        [B, 3, H, W] in [-1, 1] (what hier.encode_photo took) -- the image returned and written is then
        composite(decoded, source_image, keep, blend_hi, blend_lo): the decoder's pixels inside the edited cells, the
        photo's own farther than blend_lo pixels from them.  The keep mask is left in self.edit_keep (uint8 [B, 512]) so
        that composite can be called again with other radii; sampling and the index lists are the same either way."""
        refine_kw = dict(refine_temp=refine_temp, refine_top_k=refine_top_k, refine_top_p=refine_top_p)
        options.refine_values(refine_temp, refine_top_k, refine_top_p, batch=self.batch_size)  # (before anything is drawn)
        recolor = options.recolor_settings(self.opt)  # (options: recolor_*; None: off)
        if source_image is not None:
            source_image = self._composite_source(source_image, self.batch_size, blend_hi, blend_lo)
        keep = self.region_keep(region, labels)
        self.edit_keep = keep
        keep_rows = keep.reshape(-1).contiguous()
        bot = None
        if bot_indices_list is not None:
            bot = self._token_lists(bot_indices_list, 'edit_and_refine (bot_indices_list)')
            tex = self._texture_tokens(self.texture_mask).reshape(-1)
            err = ops.edit_prefill(bot, tex, keep_rows, 0, self.P['bot.books'].shape[1])  # (check only)
            engine._init_check(err, keep_rows, self.shape[0] * self.shape[1])
        top = self.resample_fn(top_indices_list, keep, temp=temp, order=order, rounds=rounds, choice_temp=choice_temp,
                               top_k=top_k, top_p=top_p)
        want_files = not (save_dir is None and img_name is None)
        bot_keep = (bot, keep_rows) if bot is not None else None
        if not want_files:
            keep_b, keep_mask = self.batch_size, self.texture_mask
            t_len = self.shape[0] * self.shape[1]
            self.batch_size, self.texture_mask = 1, self.texture_mask[:1]
            try:
                one = (bot[:, :t_len].contiguous(), keep_rows[:t_len]) if bot is not None else None
                img, _, inter = self.decode_indices([t[:1] for t in top], return_inter=True, bot_keep=one,
                                                    **self._refine_first_image(refine_kw))
            finally:
                self.batch_size, self.texture_mask = keep_b, keep_mask
            self._edit_results(top, inter, 1)
            if recolor is not None:  # (before the paste: the photo outside the edit keeps its pixels)
                img, _ = self._recolor_by_options(img, recolor, first=1)
            if source_image is not None:
                img, _ = ops.composite_region(img, source_image[:1], keep[:1], self.shape, r_hi=blend_hi, r_lo=blend_lo)
            return img
        img, u8, inter = self.decode_indices(top, want_u8=True, return_inter=True, bot_keep=bot_keep, **refine_kw)
        self._edit_results(top, inter, self.batch_size)
        if recolor is not None:
            img, u8 = self._recolor_by_options(img, recolor, want_u8=True)
        if source_image is not None:
            _, u8 = ops.composite_region(img, source_image, keep, self.shape, r_hi=blend_hi, r_lo=blend_lo, want_u8=True)
        save_u8_images(u8, save_dir, img_name)
        return u8

    def _composite_source(self, source_image, b, blend_hi, blend_lo):
        """checks of composite / edit_and_refine(source_image=...) -> the photo on the device, f32, contiguous"""
        ops._check_composite_radii(blend_hi, blend_lo, names=('blend_hi', 'blend_lo'))
        hh, ww = self.texture_mask.shape[2], self.texture_mask.shape[3]
        if not torch.is_tensor(source_image) or tuple(source_image.shape) != (b, 3, hh, ww):
            got = tuple(source_image.shape) if torch.is_tensor(source_image) else type(source_image).__name__
            raise ValueError(f'source_image must be [{b}, 3, {hh}, {ww}] (the photo the indices were encoded from, in '
                             f'[-1, 1]), got {got}')
        return source_image.to(self.device, torch.float32).contiguous()

    @torch.no_grad()
    def composite(self, img, source_image, keep, blend_hi=4, blend_lo=32, want_u8=False):
        """Pastes a decoded edit back into its photo (ops.composite_region).  img: f32 [B, 3, H, W] in
        [0, 1] from decode_indices / edit_and_refine (not an upscale=True image); source_image: the photo, f32
        [B, 3, H, W] in [-1, 1]; keep: uint8 [B, 512] (region_keep, or self.edit_keep after edit_and_refine).
        -> (img f32 [B, 3, H, W], u8 [B, H, W, 3] or None): img's pixels inside the edited cells, the photo's
        ((x + 1) / 2).clamp(0, 1) farther than blend_lo pixels from them, both bit for bit; in between the photo plus
        the decoder's low-frequency offset fading over blend_lo pixels and its fine detail over blend_hi."""
        b = self.batch_size
        src = self._composite_source(source_image, b, blend_hi, blend_lo)
        if not torch.is_tensor(img) or tuple(img.shape) != tuple(src.shape):
            got = tuple(img.shape) if torch.is_tensor(img) else type(img).__name__
            raise ValueError(f'img must be [{b}, 3, {src.shape[2]}, {src.shape[3]}] like the source image (upscale=True '
                             f'images are not composited), got {got}')
        n_tok = self.shape[0] * self.shape[1]
        if not torch.is_tensor(keep) or tuple(keep.shape) != (b, n_tok):
            got = tuple(keep.shape) if torch.is_tensor(keep) else type(keep).__name__
            raise ValueError(f'keep must be [{b}, {n_tok}], got {got}')
        return ops.composite_region(img.to(self.device, torch.float32).contiguous(), src,
                                    keep.to(self.device, torch.uint8).contiguous(), self.shape, r_hi=blend_hi,
                                    r_lo=blend_lo, want_u8=want_u8)

    # ---- garment colour control: an image-space operator on a decoded image and the current parsing
    # map.  Tokens, index lists and the generator are what they were.
    def _recolor_inputs(self, img, name):
        """-> (img f32 contiguous on the device, segm f32 [B, H, W]) of garment_colors / recolor"""
        segm = self.segm.to(self.device, torch.float32)
        b, hh, ww = segm.shape[0], segm.shape[-2], segm.shape[-1]
        segm = segm.reshape(b, hh, ww).contiguous()
        if not torch.is_tensor(img) or tuple(img.shape) != (b, 3, hh, ww):
            got = tuple(img.shape) if torch.is_tensor(img) else type(img).__name__
            raise ValueError(f'{name}: img must be [{b}, 3, {hh}, {ww}] like the parsing map (upscale=True images are not '
                             f'recoloured), got {got}')
        return img.to(self.device, torch.float32).contiguous(), segm

    @torch.no_grad()
    def garment_colors(self, img):
        """What colour did it draw?  img: f32 [B, 3, H, W] in [0, 1] (decode_indices / sample_and_refine).  -> dict of
        'upper' / 'lower' / 'outer': (rgb f32 [B, 3], count int64 [B]) on the device, over the pixels of that garment in
        the current self.segm (ops.region_color_stats): rgb is the inverse transform of the mean (Y, U, V), zeros where
        count is 0."""
        img, segm = self._recolor_inputs(img, 'garment_colors')
        names = list(options.RECOLOR_NAMES)
        st = ops.region_color_stats(img, segm, names)
        return {n: (ops.recolor_rgb(st[:, g, 1:4]).to(torch.float32), st[:, g, 0].to(torch.int64))
                for g, n in enumerate(names)}

    @torch.no_grad()
    def recolor(self, img, upper=None, lower=None, outer=None, labels=None, like=None, luma=1.0, gain_max=4.0, feather=2,
                want_u8=False):
        """The same outfit, a garment in another colour (ops.recolor_region) -- an operator on the
        decoded image, not a new sample.  img: f32 [B, 3, H, W] in [0, 1]; upper / lower / outer: an (r, g, b) in
        [0, 1] or a [B, 3] tensor (one colour per image) for the garment of that name in the current self.segm;
        labels = {'name': ([ids], colour)} adds a group of explicit parsing labels.  The garment's mean colour moves to
        the target (its luma by the share `luma`), its pattern and shading stay; the change fades over `feather` pixels.
        like = (image f32 [B or 1, 3, H, W] in [-1, 1], its parsing map): the target of every group named (value True)
        is the statistics of the same group in that image -- mean and, within [1 / gain_max, gain_max], contrast.  A
        group absent from an image (or from `like`) leaves that image untouched there; pixels farther than `feather`
        from every group keep their bits.  -> (img f32 [B, 3, H, W], u8 [B, H, W, 3] or None)."""
        img, segm = self._recolor_inputs(img, 'recolor')
        b = img.shape[0]
        named = [(n, ops.RECOLOR_GROUPS[n], v) for n, v in zip(options.RECOLOR_NAMES, (upper, lower, outer)) if v is not None]
        for n, entry in (labels or {}).items():
            if not isinstance(entry, (tuple, list)) or len(entry) != 2:
                raise ValueError(f'recolor: labels[{n!r}] must be ([label ids], colour), got {entry!r}')
            named.append((n, entry[0], entry[1]))
        if not named:
            raise ValueError('recolor: name at least one group (upper / lower / outer / labels)')
        groups = [ids for _, ids, _ in named]
        ops.recolor_group_bits(groups)
        ops._check_recolor_params(luma, gain_max, feather)
        if like is not None:
            if any(v is not True for _, _, v in named):
                raise ValueError('recolor: with like=(image, segm) a group is named by True, its target comes from that image')
            if not isinstance(like, (tuple, list)) or len(like) != 2 or not all(torch.is_tensor(t) for t in like):
                raise ValueError('recolor: like must be (image [B or 1, 3, H, W] in [-1, 1], its parsing map)')
            ex = like[0].to(self.device, torch.float32).contiguous()
            if ex.dim() != 4 or ex.shape[0] not in (1, b) or ex.shape[1] != 3 or like[1].numel() != ex.shape[0] * ex.shape[2] * ex.shape[3]:
                raise ValueError(f'recolor: like must be (image [{b} or 1, 3, H, W], a parsing map of its size), got '
                                 f'{tuple(like[0].shape)} and {tuple(like[1].shape)}')
            ex_segm = like[1].to(self.device, torch.float32).reshape(ex.shape[0], ex.shape[2], ex.shape[3]).contiguous()
            dst = ops.region_color_stats(ex, ex_segm, groups, img_signed=True).expand(b, -1, -1).contiguous()
            src = ops.region_color_stats(img, segm, groups)
        else:
            colours = []
            for n, _, v in named:
                if torch.is_tensor(v):
                    if tuple(v.shape) != (b, 3):
                        raise ValueError(f'recolor: the colours of {n} must be [{b}, 3], got {tuple(v.shape)}')
                    colours.append(v.to(self.device, torch.float64))
                else:
                    c = options.recolor_colour(v, f'recolor ({n})')
                    colours.append(torch.tensor(c, dtype=torch.float64, device=self.device).expand(b, 3))
            src = ops.region_color_stats(img, segm, groups)
            dst = src.clone()  # (n and the deviations are the source's: gains 1, an absent group stays absent)
            dst[:, :, 1:4] = ops.recolor_yuv(torch.stack(colours, 1))
        return ops.recolor_region(img, segm, groups, src, dst, luma=luma, gain_max=gain_max, feather=feather,
                                  want_u8=want_u8)

    def _recolor_by_options(self, img, settings, first=None, want_u8=False):
        """the options `recolor_*` (options.recolor_settings) on a decoded image; first: the image is the first `first`
        images of the batch"""
        colours, feather, luma = settings
        keep_segm = self.segm
        if first is not None:
            self.segm = self.segm[:first]
        try:
            return self.recolor(img, luma=luma, feather=feather, want_u8=want_u8, **colours)
        finally:
            self.segm = keep_segm

    def _edit_results(self, top, inter, b):
        bot = torch.cat([d['bot_lists'] for d in inter], 1) if len(inter) > 1 else inter[0]['bot_lists']
        self.edit_top_indices_list = top
        self.edit_bot_indices_list = [bot[i].view(b, -1) for i in range(bot.shape[0])]

    def _exact_sampler(self):
        """The same transformer on the exact-fp32 matrix instructions (built on first use; shares the weights)."""
        if getattr(self, '_sampler_exact', None) is None:
            self._sampler_exact = engine.SamplerNet(self.P, self._tf_desc, self.opt['bert_n_head'], 'tf', split=False)
        return self._sampler_exact

    # ------------------------------------------------------------ stage R
    def _top_quant_rows(self, top_lists, tex_tok):
        """R-1/R-2: texture-routed gather + top_post_quant_conv -> rows [B*512, 256]."""
        P = self.P
        zq = ops.codebook_gather_tex(top_lists, tex_tok.reshape(-1), P['top.books'])
        return ops.gemm(zq, P['top.pq.w'], bias=P['top.pq.b'])

    def _head_features(self, top_quant_rows, b):
        """R-3: UNet -> all 18 head convs as one GEMM -> rows [b*512, 18 * cf]."""
        P = self.P
        h, w = self.shape
        feat, _, _ = self.index_pred_guidance_encoder.forward(top_quant_rows, b, h, w)
        return ops.conv3x3(feat, P['ipd.conv.w'], b, h, w, feat.shape[1], bias=P['ipd.conv.b'], act=ACT_RELU)

    def _bot_indices(self, top_quant_rows, tex_tok, b, refine=None, row0=0):
        """R-3 batched: UNet -> all 18 head convs as one GEMM -> routed 1x1 + argmax.  refine (RefineDraw; None: the
        reference's argmax): the index of every token is drawn instead (t2h_routed_head_sample), these b images being
        token rows row0 .. row0 + b*512 - 1 of the draw's batch."""
        P = self.P
        hc = self._head_features(top_quant_rows, b)
        if refine is None:
            return ops.routed_head_argmax(hc, P['ipd.seg.w'], P['ipd.seg.b'], tex_tok.reshape(-1),
                                          self.ipd['n_heads'], self.ipd['cf'], self.ipd['n_class'])
        t_len = self.shape[0] * self.shape[1]
        if refine.table is not None:
            rules = dict(params=refine.table[row0 // t_len:row0 // t_len + b], rows_per_sample=t_len)
        else:
            rules = dict(zip(('temp', 'top_k', 'top_p'), refine.values))
        if refine.philox is not None:
            noise = dict(philox=refine.philox, noise_rows=refine.rows, noise_row0=row0)
        else:
            noise = dict(expo=refine.expo[row0:row0 + b * t_len])
        return ops.routed_head_sample(hc, P['ipd.seg.w'], P['ipd.seg.b'], tex_tok.reshape(-1).contiguous(),
                                      self.ipd['n_heads'], self.ipd['cf'], self.ipd['n_class'], **rules, **noise)

    def _refine_options(self):
        """refine_temp / refine_top_k / refine_top_p of the options as keyword arguments ({}: absent, the argmax)."""
        vals = options.refine_sampling(self.opt)
        return dict(zip(options.REFINE_KEYS, vals)) if vals is not None else {}

    @staticmethod
    def _refine_first_image(kw):
        """the refine arguments of a batch, for a decode of its first image alone"""
        return {k: ([options.per_image_values(len(v), v, k)[0]] if options.is_per_image(v) else v) for k, v in kw.items()}

    def _refine_draw(self, batch, refine_temp, refine_top_k, refine_top_p):
        """-> None (nothing set: the argmax, the generator is not touched) or the RefineDraw of a decode of `batch`
        images.  The arguments are validated first (ValueError); then the generator is read ONCE and advanced by one
        [batch * 512, n_class] exponential_ draw -- every chunk, and a re-run after an overflow, uses this draw."""
        vals = options.refine_values(refine_temp, refine_top_k, refine_top_p, batch=batch)
        if vals is None:
            return None
        n_class = self.ipd['n_class']
        sp = ops.sampling_params(batch, *vals, n_class=n_class)
        table = ops.sample_params_tensor(sp.table, self.device) if sp.table is not None else None
        n = batch * self.shape[0] * self.shape[1]
        src = self.noise if self.noise is not None else engine.TorchDeviceNoise(self.device)
        philox = expo = None
        if isinstance(src, engine.TorchDeviceNoise) and src.emulation_ok(n, n_class):
            gen, _ = src.generator()
            philox = (gen.initial_seed(), gen.get_offset())
            gen.set_offset(philox[1] + ops.torch_draw_geometry(n * n_class, self.device)[1])
        else:  # (another noise source, or a torch build whose Philox draws the kernels do not reproduce)
            expo = src.exponential(0, 0, (n, n_class)).to(self.device, torch.float32).contiguous()
        return RefineDraw(vals, table, philox, expo, n)

    @torch.no_grad()
    def bot_index_prediction(self, feature_top, texture_mask, refine_temp=None, refine_top_k=None, refine_top_p=None):
        """models/sample_model.py:183-213.  feature_top f32 [B,256,32,16] (NCHW,
        as the reference passes it) -> list of 18 int64 [B,32,16].  refine_temp / refine_top_k / refine_top_p: see
        decode_indices."""
        b = feature_top.shape[0]
        refine = self._refine_draw(b, refine_temp, refine_top_k, refine_top_p)
        tex_tok = self._texture_tokens(texture_mask.to(self.device))
        rows = ops.nchw_to_nhwc(feature_top.to(self.device, torch.float32))
        lists = self._bot_indices(rows, tex_tok, b, refine=refine)
        return [lists[i].view(b, self.shape[0], self.shape[1]) for i in range(lists.shape[0])]

    # ------------------------------------------------------------ stage D
    def _decode(self, top_lists, tex_tok, b, want_u8=False, return_inter=False, upscale=False, bot_keep=None,
                refine=None, row0=0):
        """sample_and_refine body after sample_fn (models/sample_model.py:220-246),
        batched.  top_lists int64 [18, b*512].  bot_keep = (bot_lists [18, b*512], keep uint8 [b*512]): the
        predicted bottom indices are replaced by those where keep (region editing).  refine / row0: see _bot_indices."""
        P = self.P
        h, w = self.shape
        top_quant = self._top_quant_rows(top_lists, tex_tok)
        bot_lists = self._bot_indices(top_quant, tex_tok, b, refine=refine, row0=row0)
        if bot_keep is not None:
            ops.merge_kept_indices(bot_keep[0], bot_keep[1], bot_lists)
        quant_bot = ops.codebook_gather_fold(bot_lists, tex_tok.reshape(-1), P['bot.books'], b, h, w)
        quant_bot = ops.gemm(quant_bot, P['bot.pq.w'], bias=P['bot.pq.b'])
        bot_h = self.bot_decoder_res.decode_res(quant_bot, b, 2 * h, 2 * w, upscale=upscale)
        dec, ho, wo = self.decoder.decode(top_quant, b, h, w, bot_h=bot_h, upscale=upscale)
        img, u8 = ops.image_epilogue(dec, b, ho, wo, want_u8=want_u8)
        if return_inter:
            return img, u8, dict(top_quant=top_quant, bot_lists=bot_lists, bot_h=bot_h, dec=dec)
        return img, u8

    @torch.no_grad()
    def decode_indices(self, top_indices_list, want_u8=False, return_inter=False, upscale=False, bot_keep=None,
                       refine_temp=None, refine_top_k=None, refine_top_p=None):
        """Batched refine + decode of sampled top indices (list of 18 [B,512]).
        upscale=True: 1024x512 output -- both quantised latents are nearest-x2
        upsampled before the (fully convolutional) decoders, the interpretation
        of BASELINE.json configs[4] given in SURVEY.md 8(d).  bot_keep (region editing, edit_and_refine): see
        _decode.  refine_temp / refine_top_k / refine_top_p (not in the reference): any of them set
        DRAWS the bottom (detail) index of every token from the index-prediction head's softmax at refine_temp (default
        1), among the refine_top_k most likely codes / the most likely codes holding refine_top_p of the probability,
        instead of taking its mode; each a scalar or a sequence with one entry per image.  Such a call consumes torch's
        GPU generator as ONE [B*512, n_class] exponential_ draw; with all three None the generator is not touched."""
        # the draw is fixed BEFORE the first attempt: the re-run below uses the same (seed, offset), and the generator
        # is advanced once
        refine = self._refine_draw(self.batch_size, refine_temp, refine_top_k, refine_top_p)
        try:
            return self._decode_indices(top_indices_list, want_u8, return_inter, upscale, bot_keep, refine)
        except engine.SplitOverflowError as e:
            # (once more, convolutions on the exact-fp32 kernels)
            if not _overflow_fallback('VQGAN refine / decode', 'T2H_SPLIT_CONV', e):
                raise
            keep = self.decoder.use_split, self.bot_decoder_res.use_split
            self.decoder.use_split = self.bot_decoder_res.use_split = False
            try:
                return self._decode_indices(top_indices_list, want_u8, return_inter, upscale, bot_keep, refine)
            finally:
                self.decoder.use_split, self.bot_decoder_res.use_split = keep

    def _decode_indices(self, top_indices_list, want_u8, return_inter, upscale, bot_keep=None, refine=None):
        b = self.batch_size
        tex_tok = self._texture_tokens(self.texture_mask)
        top = torch.stack([t.reshape(-1) for t in top_indices_list]).contiguous()
        imgs, u8s, inters = [], [], []
        t_len = self.shape[0] * self.shape[1]
        chunk = max(1, DECODE_CHUNK // (4 if upscale else 1))
        for s in range(0, b, chunk):
            e = min(b, s + chunk)
            bk = ((bot_keep[0][:, s * t_len:e * t_len].contiguous(), bot_keep[1][s * t_len:e * t_len])
                  if bot_keep is not None else None)
            res = self._decode(top[:, s * t_len:e * t_len].contiguous(), tex_tok[s:e], e - s,
                               want_u8=want_u8, return_inter=return_inter, upscale=upscale, bot_keep=bk,
                               refine=refine, row0=s * t_len)
            imgs.append(res[0])
            u8s.append(res[1])
            if return_inter:
                inters.append(res[2])
        if self.split_conv and self.decoder.use_split:  # split-precision convolutions: loud on fp16-range overflow
            engine.check_split_overflow('VQGAN refine / decode', knob='T2H_SPLIT_CONV')
        img = torch.cat(imgs, 0) if len(imgs) > 1 else imgs[0]
        u8 = (torch.cat(u8s, 0) if len(u8s) > 1 else u8s[0]) if want_u8 else None
        if return_inter:
            return img, u8, inters
        return img, u8

    @torch.no_grad()
    def sample_and_refine(self, save_dir=None, img_name=None, seeds=None):
        """models/sample_model.py:215-254.  With both arguments None returns the
        first sample as f32 [1,3,512,256] in [0,1] (what ui_demo.py:162 uses);
        otherwise writes {save_dir}/{img_name[i]} PNGs.  seeds (options: per_image_seeds, derived by inference();
        DESIGN.md 4.6h): the top indices of image b are sample_fn's with seeds[b].  With the option `revise_passes` > 0
         the sampled map goes through revise_fn -- `revise_fraction`, `revise_folds`, the run's
        truncation / order settings and `seeds` -- before the bottom indices are predicted."""
        if seeds is not None:
            seeds = options.image_seeds(self.batch_size, seeds)
            options.per_image_seeding(dict(self.opt, per_image_seeds=True))  # (the options that cannot keep the promise)
        confidence = self._confidence_options()
        top_k, top_p = self._truncation_options()  # (options: sample_top_k / sample_top_p)
        trunc = {k: v for k, v in (('top_k', top_k), ('top_p', top_p)) if v is not None}
        refine_kw = self._refine_options()  # (options: refine_temp / refine_top_k / refine_top_p)
        best_of = options.sampling_best_of(self.opt)  # (options: sample_best_of; 1: the calls below, as always)
        revise = options.revise_settings(self.opt)  # (options: revise_passes / revise_fraction / revise_folds; None: off)
        recolor = options.recolor_settings(self.opt)  # (options: recolor_*; None: off -- the image is the decoder's)
        if best_of > 1:
            kw = dict(trunc, temp=1)
            if confidence is not None:
                kw.update(rounds=confidence[0], choice_temp=confidence[1])
            else:
                kw.update(sample_steps=self.sample_steps)
            sampled_top_indices_list, _, score, choice = self.sample_best_of(
                best_of, order='confidence' if confidence is not None else 'random', **kw)
            for i, (c, s) in enumerate(zip(choice.tolist(), score.tolist())):
                logger.info(f'best of {best_of}: image {i} keeps candidate {c} (mean log-probability per token {s:.4f})')
        elif confidence is not None:  # (options: sample_order: confidence)
            sampled_top_indices_list = self.sample_fn_confidence(rounds=confidence[0], temp=1, choice_temp=confidence[1],
                                                                 **trunc)
        elif trunc or seeds is not None:
            seed_kw = dict(seeds=seeds) if seeds is not None else {}
            sampled_top_indices_list = self.sample_fn(temp=1, sample_steps=self.sample_steps, **trunc, **seed_kw)
        else:
            sampled_top_indices_list = self.sample_fn(temp=1, sample_steps=self.sample_steps)
        if revise is not None:  # (options: revise_passes > 0)
            kw = dict(trunc, temp=1, sample_steps=self.sample_steps)
            if confidence is not None:
                kw.update(order='confidence', rounds=confidence[0], choice_temp=confidence[1])
            if seeds is not None:
                kw.update(seeds=seeds)
            sampled_top_indices_list = self.revise_fn(sampled_top_indices_list, passes=revise[0], fraction=revise[1],
                                                      folds=revise[2], **kw)
        want_files = not (save_dir is None and img_name is None)
        if not want_files:
            keep_b, keep_mask = self.batch_size, self.texture_mask
            self.batch_size, self.texture_mask = 1, self.texture_mask[:1]
            try:
                img, _ = self.decode_indices([t[:1] for t in sampled_top_indices_list],
                                             **self._refine_first_image(refine_kw))
            finally:
                self.batch_size, self.texture_mask = keep_b, keep_mask
            if recolor is not None:  # (options: recolor_upper / recolor_lower / recolor_outer)
                img, _ = self._recolor_by_options(img, recolor, first=1)
            return img
        img, u8 = self.decode_indices(sampled_top_indices_list, want_u8=True, **refine_kw)
        if recolor is not None:
            _, u8 = self._recolor_by_options(img, recolor, want_u8=True)
        save_u8_images(u8, save_dir, img_name)

    def _image_seeds(self, img_name):
        """{} or dict(seeds=...): with the option `per_image_seeds`, options.image_seed of (manual_seed, name) per image"""
        if not options.per_image_seeding(self.opt):
            return {}
        if self.opt['manual_seed'] is None:
            raise ValueError('per_image_seeds derives every image\'s seed from manual_seed: set it')
        return dict(seeds=[options.image_seed(self.opt['manual_seed'], name) for name in img_name])

    def inference(self, data_loader, save_dir):
        for _, data in enumerate(data_loader):
            img_name = data['img_name']
            self.feed_data(data)
            self.sample_and_refine(save_dir, img_name, **self._image_seeds(img_name))


_warned = set()


def _overflow_fallback(stage, knob, err, to='exact-fp32'):
    """True: re-run the stage on the `to` kernels (default; warns once per stage).  T2H_OVERFLOW_FALLBACK=0:
    the SplitOverflowError propagates, as before."""
    if os.environ.get('T2H_OVERFLOW_FALLBACK', '1') == '0':
        return False
    if stage not in _warned:
        _warned.add(stage)
        import warnings
        warnings.warn(f'text2human_amd: {err}  Re-running the {stage} on the {to} kernels; '
                      f'set {knob}=0 to start there, T2H_OVERFLOW_FALLBACK=0 to raise instead.')
    return True


def save_u8_images(u8, save_dir, img_name):
    """torchvision.utils.save_image(dec, path, nrow=1, padding=4) of a single
    image == its uint8 HWC PNG (models/sample_model.py:250-254)."""
    from PIL import Image
    arr = u8.cpu().numpy()
    for i in range(arr.shape[0]):
        Image.fromarray(arr[i]).save(os.path.join(save_dir, img_name[i]))


class SampleFromParsingModel(BaseSampleModel):
    """SampleFromParsing model (models/sample_model.py:343-360)."""

    def feed_data(self, data):
        self.segm = data['segm'].to(self.device)
        self.texture_mask = data['texture_mask'].to(self.device)
        self.batch_size = self.segm.size(0)
        self.segm_tokens = self.get_quantized_segm(self.segm)
        self.segm_tokens = self.segm_tokens.view(self.batch_size, -1)


class SampleFromPoseModel(BaseSampleModel):
    """SampleFromPose model (models/sample_model.py:363-498)."""

    def __init__(self, opt, state_dicts=None):
        super().__init__(opt, state_dicts)
        self.palette = [[0, 0, 0], [255, 250, 250], [220, 220, 220], [250, 235, 215],
                        [255, 250, 205], [211, 211, 211], [70, 130, 180], [127, 255, 212],
                        [0, 100, 0], [50, 205, 50], [255, 255, 0], [245, 222, 179],
                        [255, 140, 0], [255, 0, 0], [16, 78, 139], [144, 238, 144],
                        [50, 205, 174], [50, 155, 250], [160, 140, 88], [213, 140, 88],
                        [90, 140, 90], [185, 210, 205], [130, 165, 180], [225, 141, 151]]

    def _pack(self, sds):
        super()._pack(sds)
        P = self.P
        self.shape_emb = weights.pack_shape_embedder(P, sds['shape_embedder'], 'semb',
                                                     self.opt['shape_attr_class_num'])
        d_su = weights.pack_unet(P, sds['shape_encoder'], 'sunet',
                                 attr_channels=self.opt['shape_embedder_out_dim'])
        self.shape_parsing_encoder = engine.UNetStack(P, 'sunet', d_su)
        self.shape_head = weights.pack_fcn_head(P, sds['shape_decoder'], 'shead')

    def feed_data(self, data):
        self.pose = data['densepose'].to(self.device)
        self.batch_size = self.pose.size(0)
        self.shape_attr = data['shape_attr'].to(self.device)
        self.upper_fused_attr = data['upper_fused_attr'].to(self.device)
        self.lower_fused_attr = data['lower_fused_attr'].to(self.device)
        self.outer_fused_attr = data['outer_fused_attr'].to(self.device)

    def inference(self, data_loader, save_dir):
        for _, data in enumerate(data_loader):
            img_name = data['img_name']
            self.feed_data(data)
            self.generate_parsing_map()
            self.generate_quantized_segm()
            self.generate_texture_map()
            self.sample_and_refine(save_dir, img_name, **self._image_seeds(img_name))

    def _attr_embedding(self, shape_attr):
        """ShapeAttrEmbedding.forward (shape_attr_embedding_arch.py:23-35)."""
        return ops.shape_attr_embed(shape_attr.long().contiguous(), self.shape_emb)

    @torch.no_grad()
    def generate_parsing_map(self):
        """models/sample_model.py:431-437 -> self.segm int64 [B,1,H,W]."""
        P = self.P
        b, _, hh, ww = self.pose.shape
        attr = self._attr_embedding(self.shape_attr)
        cin_pad = P['sunet.enc.0.0.w'].shape[1] // 9
        x = ops.nchw_to_nhwc(self.pose.to(torch.float32), cpad=cin_pad)
        feat, h, w = self.shape_parsing_encoder.forward(x, b, hh, ww, attr=attr)
        y = ops.conv3x3(feat, P['shead.conv.w'], b, h, w, feat.shape[1], bias=P['shead.conv.b'],
                        act=ACT_RELU)
        logits = ops.gemm(y, P['shead.seg.w'], bias=P['shead.seg.b'])
        self.seg_logits_rows = logits
        self.segm = ops.argmax_rows(logits).view(b, 1, h, w)

    def generate_quantized_segm(self):
        self.segm_tokens = self.get_quantized_segm(self.segm)
        self.segm_tokens = self.segm_tokens.view(self.batch_size, -1)

    def generate_texture_map(self):
        """models/sample_model.py:443-467."""
        self.texture_mask = ops.texture_map(self.segm.contiguous(),
                                            self.upper_fused_attr.long().contiguous(),
                                            self.lower_fused_attr.long().contiguous(),
                                            self.outer_fused_attr.long().contiguous())

    def feed_pose_data(self, pose_img):
        self.pose = pose_img.to(self.device)
        self.batch_size = self.pose.size(0)

    def feed_shape_attributes(self, shape_attr):
        self.shape_attr = shape_attr.to(self.device)

    def feed_texture_attributes(self, texture_attr):
        self.upper_fused_attr = texture_attr[0].unsqueeze(0).to(self.device)
        self.lower_fused_attr = texture_attr[1].unsqueeze(0).to(self.device)
        self.outer_fused_attr = texture_attr[2].unsqueeze(0).to(self.device)

    def palette_result(self, result):
        seg = result[0]
        palette = np.array(self.palette)
        color_seg = np.zeros((seg.shape[0], seg.shape[1], 3), dtype=np.uint8)
        for label, color in enumerate(palette):
            color_seg[seg == label, :] = color
        return color_seg
