"""Region editing on the GPU (-m gpu; DESIGN.md, "Editing a region"): resample_fn / edit_and_refine against the
reference's loop started from a partially known state, restated below on the oracle (oracle/torch_ref.py), with
synthetic checkpoints."""
import os

import numpy as np
import pytest
import torch

from oracle import torch_ref as R
from text2human_amd import defaults, engine, ops, options, synthetic
from text2human_amd._lib import T2HError
from text2human_amd.models import SampleFromParsingModel

from parity_util import ACT_TOL, RecordingNoise, account, odev, osds, seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LABELS = (1, 2, 3)   # parsing labels of synthetic.parsing_batch's coarse cells: about 1/8 of the rows


def edit_loop(segm_tok, tex_tok, sd, steps, src, keep, noise, temp=1.0, mask_id=18432, trace=None):
    """BaseSampleModel.sample_fn (models/sample_model.py:256-328) with the edit's initial state:
    x_t = keep ? src[tex] + 1024 tex : mask_id, unmasked = keep, out = the kept tokens.  src [18, n], keep [n]."""
    b, T = tex_tok.shape
    n = b * T
    tex = tex_tok.reshape(-1)
    k = keep.reshape(-1).bool()
    own = src[tex, torch.arange(n, device=tex.device)]
    x_t = torch.where(k, own + 1024 * tex, torch.full_like(own, mask_id)).view(b, T)
    unmasked = k.view(b, T).clone()
    out = [torch.where(k & (tex == h), src[h], torch.full_like(own, -1)) for h in range(18)]
    if trace is not None:
        trace.append(dict(t=steps + 1, x_t=x_t.clone(), active=[]))
    for t in range(steps, 0, -1):
        changes = noise.uniform(t, (b, T)) < 1.0 / float(t)
        changes = torch.bitwise_xor(changes, torch.bitwise_and(changes, unmasked))
        unmasked = torch.bitwise_or(unmasked, changes)
        ch = changes.view(-1)
        active = [cb for cb in range(18) if bool((tex[ch] == cb).sum() > 0)]
        logits = R.transformer_logits(x_t, segm_tok, tex_tok, sd, heads=set(active)) if active else None
        x_flat = x_t.view(-1).clone()
        for cb in active:
            lg = logits[cb] / temp
            expo = noise.exponential(t, cb, (n, lg.shape[-1]))
            x0 = R.categorical_argmax(lg.reshape(n, -1), expo)
            sel = torch.bitwise_and(ch, tex == cb)
            x_flat[sel] = x0[sel] + 1024 * cb
            out[cb][sel] = x0[sel]
        x_t = x_flat.view(b, T)
        if trace is not None:
            trace.append(dict(t=t, x_t=x_t.clone(), active=active))
    return [o.view(b, T) for o in out]


@pytest.fixture(scope='module')
def opt():
    return options.dict_to_nonedict(defaults.sample_from_parsing())


@pytest.fixture(scope='module')
def sds(opt):
    return synthetic.make_state_dicts(opt, seed=77)


@pytest.fixture(scope='module')
def model(opt, sds):
    return SampleFromParsingModel(opt, state_dicts=sds)


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def _source(model, B, steps, seed):
    """a batch fed to the model and a sample of it to edit (18 x [B, 512])"""
    model.feed_data(synthetic.parsing_batch(B, seed=seed))
    seed_all(seed)
    return model.sample_fn(temp=1, sample_steps=steps)


@pytest.mark.parametrize('graph,shrink', [('1', '1'), ('1', '0'), ('0', '1'), ('0', '0')])
def test_keep_all_zero_is_sample_fn(model, monkeypatch, graph, shrink):
    monkeypatch.setenv('T2H_GRAPH', graph)
    monkeypatch.setenv('T2H_SHRINK_BATCH', shrink)
    B, steps = 4, 64
    src = _source(model, B, steps, seed=31)
    seed_all(5)
    want = torch.stack(model.sample_fn(temp=1, sample_steps=steps))
    off_want, mode_want = _gen().get_offset(), model.sampler_fn.last_launch_mode
    seed_all(5)
    got = torch.stack(model.resample_fn(src, torch.zeros(B, 512, dtype=torch.uint8), sample_steps=steps))
    assert torch.equal(got, want) and _gen().get_offset() == off_want
    assert model.sampler_fn.last_launch_mode == mode_want == ('graph' if graph == '1' else 'eager')


def test_keep_all_ones_returns_the_source_and_only_moves_the_generator_by_the_rand_draws(model):
    B, steps = 2, 40
    src = _source(model, B, steps, seed=32)
    seed_all(6)
    off0 = _gen().get_offset()
    got = model.resample_fn(src, torch.ones(B, 512, dtype=torch.uint8), sample_steps=steps)
    assert torch.equal(torch.stack(got), torch.stack(src))
    assert model.sampler_fn.last_stats['rounds'] == 0 and model.sampler_fn.last_stats['rows_kept'] == B * 512
    assert _gen().get_offset() - off0 == steps * ops.torch_draw_geometry(B * 512)[1]


def test_partial_region_matches_the_restated_loop_on_cpu_noise(model, sds):
    B, steps = 2, 4
    src = _source(model, B, steps, seed=33)
    keep = model.region_keep(labels=LABELS)
    assert 0 < int(keep.sum()) < B * 512
    model.noise = R.SeededNoise(3, 'cpu')
    try:
        got = torch.stack(model.resample_fn(src, keep, sample_steps=steps)).cpu()
    finally:
        model.noise = None
    tex = R.texture_tokens(model.texture_mask.cpu())
    with torch.no_grad():
        ref = edit_loop(model.segm_tokens.cpu(), tex, sds['sampler'], steps, torch.stack(src).cpu().view(18, -1),
                        keep.cpu(), R.SeededNoise(3, 'cpu'))
    assert torch.equal(got, torch.stack(ref))
    k = keep.cpu().bool()
    assert torch.equal(got[:, k], torch.stack(src).cpu()[:, k])


def test_partial_region_b8_256_steps_on_the_device_generator(model, sds):
    B, steps, seed = 8, 256, 44
    src = _source(model, B, steps, seed=34)
    keep = model.region_keep(labels=LABELS)
    k = keep.view(-1).bool()
    src_t = torch.stack(src).view(18, -1)
    seed_all(seed)
    got = torch.stack(model.resample_fn(src, keep)).view(18, -1)
    rounds = model.sampler_fn.last_stats['rounds']
    assert torch.equal(got[:, k], src_t[:, k])                      # kept rows: the source, bit for bit
    sd = osds(sds)['sampler']
    tex_tok = R.texture_tokens(model.texture_mask).to(DEV)
    noise, trace = RecordingNoise(DEV), []
    seed_all(seed)
    with torch.no_grad():
        ref = torch.stack(edit_loop(model.segm_tokens, tex_tok, sd, steps, src_t, keep, noise, trace=trace)).view(18, -1)
    n_bad = int((got != ref).any(0).sum())
    predicted = steps * (1 - (1 - 1 / steps) ** (~k).view(B, -1).sum(1).max().item())
    print(f'edit B=8: {int((~k).sum())} rows resampled, {rounds} rounds (predicted <= {predicted:.0f}), '
          f'{n_bad} rows differ from the restated loop')
    if n_bad == 0:
        return
    # the first divergence cascades: force the HIP sampler onto the restated loop's trajectory and account for every
    # differing decision as a near-tie (parity_util.account, as the existing parity tests do)
    tr = {d['t']: d for d in trace}
    mism = []

    def round_hook(r, st, x_t, out):
        st_l = st.tolist()
        want = torch.stack([tr[t]['x_t'][b] if t else x_t[b] for b, t in enumerate(st_l)])
        for b, j in (x_t != want).nonzero().tolist():
            mism.append((st_l[b], b * 512 + j, int(x_t[b, j]), int(want[b, j])))
        x_t.copy_(want)

    seed_all(seed)
    engine.sample_tokens(model.sampler_fn, model.segm_tokens.contiguous(), tex_tok, steps, model.mask_id,
                         round_hook=round_hook, compact=True, init=(src_t.contiguous(), keep.view(-1).contiguous()))
    rows = account(model, sd, model.texture_mask, tr, noise.state, mism, steps + 1)
    assert all(r['explained'] for r in rows), rows


@pytest.fixture(scope='module')
def photo(opt):
    sds = synthetic.make_state_dicts(opt, seed=1234, encode=True)
    from text2human_amd.models import VQGANTextureAwareSpatialHierarchyInferenceModel as M
    return M(opt, state_dicts=sds), SampleFromParsingModel(opt, state_dicts=sds), sds


def _oracle_decode(top, bot, mask, sds):
    with torch.no_grad():
        pq, bq = sds['top_post_quant_conv'], sds['bot_post_quant_conv']
        tq = torch.nn.functional.conv2d(R.top_codebook_entry(top, mask, sds['top_quantize']), pq['weight'], pq['bias'])
        qb = torch.nn.functional.conv2d(R.bot_codebook_entry(bot, mask, sds['bot_quantize']), bq['weight'], bq['bias'])
        dec = R.decoder(tq, sds['decoder'], bot_h=R.decoder_res(qb, sds['bot_decoder_res']))
    return ((dec + 1) / 2).clamp(0, 1)


def test_photo_edit_keeps_the_encoders_indices_outside_the_region(photo, tmp_path):
    from PIL import Image
    hier, model, sds = photo
    B = 2
    batch = synthetic.parsing_batch(B, seed=77)
    img = torch.rand(B, 3, 512, 256, generator=torch.Generator().manual_seed(21)) * 2 - 1
    model.feed_data(batch)
    hier.top_encode(img, batch['texture_mask'])
    top_enc = hier.top_indices_list.view(18, B, 512).clone()
    bot_enc = torch.stack(hier.bot_encode(img, batch['texture_mask'])).view(18, B, 512)
    k = model.region_keep(labels=LABELS).bool()
    assert 0 < int(k.sum()) < B * 512
    steps = 16
    model.sample_steps = steps
    seed_all(9)
    first = model.edit_and_refine(list(top_enc), labels=LABELS, bot_indices_list=list(bot_enc))
    top0, bot0 = torch.stack(model.edit_top_indices_list), torch.stack(model.edit_bot_indices_list)
    seed_all(9)
    names = ['a.png', 'b.png']
    u8 = model.edit_and_refine(list(top_enc), labels=LABELS, bot_indices_list=list(bot_enc), save_dir=str(tmp_path),
                               img_name=names)
    top, bot = torch.stack(model.edit_top_indices_list), torch.stack(model.edit_bot_indices_list)
    model.sample_steps = defaults.sample_from_parsing()['sample_steps']
    assert torch.equal(top, top0) and torch.equal(bot[:, :1], bot0)          # same generator state -> same edit
    kk = k.unsqueeze(0).expand(18, -1, -1)
    assert torch.equal(top[kk], top_enc[kk]) and torch.equal(bot[kk], bot_enc[kk])
    assert not torch.equal(top, top_enc)                                        # the region was resampled
    ref = _oracle_decode(odev(list(top)), odev(list(bot)), odev(batch['texture_mask']), osds(sds)).cpu()
    err = (first.cpu() - ref[:1]).abs().max().item()
    assert err < ACT_TOL, err
    assert (u8.cpu().int() - R.to_uint8(ref).int()).abs().max().item() <= 1
    for i, nm in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(os.path.join(str(tmp_path), nm))), u8[i].cpu().numpy())


def test_invalid_kept_row_raises_and_changes_nothing(model):
    B = 2
    src = _source(model, B, 8, seed=35)
    lists = torch.stack(src).clone()
    tex = model._texture_tokens(model.texture_mask)
    b, j = 1, 77
    lists[tex[b, j], b, j] = -1
    keep = torch.ones(B, 512, dtype=torch.uint8)
    seg, mask = model.segm_tokens.clone(), model.texture_mask.clone()
    seed_all(3)
    off0 = _gen().get_offset()
    with pytest.raises(T2HError, match=f'token row {j} of sample {b}'):
        model.resample_fn(list(lists), keep, sample_steps=8)
    assert _gen().get_offset() == off0
    assert torch.equal(model.segm_tokens, seg) and torch.equal(model.texture_mask, mask)
    keep[b, j] = 0                                       # resampling that row makes the edit valid
    out = torch.stack(model.resample_fn(list(lists), keep, sample_steps=8))
    assert (out.gather(0, tex.unsqueeze(0)) >= 0).all()
    with pytest.raises(ValueError):
        model.region_keep(region=torch.ones(B, 1, 256, 256, dtype=torch.uint8))
    with pytest.raises(ValueError):
        model.region_keep()
    with pytest.raises(ValueError):
        model.resample_fn(src, torch.zeros(B, 256, dtype=torch.uint8))
