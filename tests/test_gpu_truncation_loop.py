"""Truncated sampling, the whole loops against torch restatements (-m gpu; DESIGN.md, "Truncated sampling").

sample_fn: the reference's loop with `logits[logits < theta] = -inf` before the race (tests/truncation_ref.py, float64),
step by step on the device's own hidden states (the logits of the state each step saw, SamplerNet.logits) and on the
same injected draws (a seeded noise source both sides read).  sample_fn_confidence: the loop of tests/confidence_ref.py
on the oracle's transformer with the threshold added to its draw, the device teacher-forced onto the restated
trajectory round by round; the commit sets stay the top-k of the kernel's own scores.

Two correct implementations whose logits differ by dl cannot agree on a kept set whose boundary lies within the band
dl opens (truncation_ref.kept_torch): rows where the strict and the permissive set have different winners are counted
as undecided, reported, and may be at most 1 % of the sampled rows; every other differing token must be a near-tie of
the race (log-score gap <= 2 dl), as in the untruncated parity tests.  dl: the measured logit difference per row where
both sides' logits exist (confidence mode); ACT_TOL / min(temp, 1) -- the documented activation tolerance, DESIGN.md
section 2 -- where the tail's own logits are not observable (sample_fn: the hook's evaluation takes another GEMM path
than the round's)."""
import pytest
import torch

import confidence_ref as CR
import truncation_ref as ref
from text2human_amd import defaults, engine, options, synthetic
from text2human_amd.models import SampleFromParsingModel

from parity_util import ACT_TOL, seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MASK_ID = 18432
SETTINGS = [dict(top_k=64), dict(top_p=0.9), dict(top_k=64, top_p=0.9)]


@pytest.fixture(scope='module')
def opt():
    return options.dict_to_nonedict(defaults.sample_from_parsing())


@pytest.fixture(scope='module')
def sds(opt):
    return synthetic.make_state_dicts(opt, seed=1234)


@pytest.fixture(scope='module')
def model(opt, sds):
    return SampleFromParsingModel(opt, state_dicts=sds)


class SeededNoise:
    """Draws that depend on (seed, step, head) only, made on the device: the engine and the restatement both ask for
    them, nothing is stored."""

    def __init__(self, seed):
        self.seed = int(seed)

    def _gen(self, step, head):
        g = torch.Generator(device=DEV)
        g.manual_seed(self.seed * 1000003 + int(step) * 64 + (int(head) + 1 if head is not None else 0))
        return g

    def uniform(self, step, shape):
        return torch.rand(shape, device=DEV, generator=self._gen(step, None))

    def exponential(self, step, head, shape):
        return torch.empty(shape, device=DEV).exponential_(1.0, generator=self._gen(step, head))


def _feed(model, B, seed):
    model.feed_data(synthetic.parsing_batch(B, seed=seed))
    return model._texture_tokens(model.texture_mask)


def _own_logits(net, x_t, segm, tex_tok, temp):
    """device logits of every row's own head / temp: [n, 1024]"""
    present = set(tex_tok.unique().tolist())
    lg = net.logits(x_t, segm, tex_tok, heads=present)
    n = tex_tok.numel()
    out = torch.zeros(n, 1024, device=DEV)
    for h in present:
        sel = tex_tok.view(-1) == h
        out[sel] = lg[h].reshape(n, -1)[sel]
    return out / temp


@pytest.mark.parametrize('kw', SETTINGS, ids=str)
@pytest.mark.parametrize('temp', [1.0, 0.7])
@pytest.mark.parametrize('B', [2, 8])
def test_sample_fn_against_the_restated_loop(model, B, temp, kw):
    steps, seed = 16, 3
    tex_tok = _feed(model, B, 60 + B)
    segm = model.segm_tokens.contiguous()
    net = model.sampler_fn
    noise = SeededNoise(seed)
    tex = tex_tok.view(-1)
    prev = [torch.full((B, 512), MASK_ID, dtype=torch.int64, device=DEV)]
    tot = dict(rows=0, equal=0, undecided=0, near_ties=0, unexplained=[])

    def hook(t, x_t, out):
        snapshot = x_t.clone()
        rows = (snapshot != prev[0]).view(-1).nonzero().flatten()
        l = _own_logits(net, prev[0], segm, tex_tok, temp)[rows]
        E = torch.empty(len(rows), 1024, device=DEV)
        for h in tex[rows].unique().tolist():      # the step's draw of that head, the rows it owns
            sel = tex[rows] == h
            E[sel] = noise.exponential(t, h, (B * 512, 1024))[rows[sel]]
        tok_dev = snapshot.view(-1)[rows] - 1024 * tex[rows]
        assert bool(((tok_dev >= 0) & (tok_dev < 1024)).all())
        dl = torch.full((len(rows), ), ACT_TOL / min(temp, 1.0), device=DEV)
        res = ref.judge_rows(l, E, tok_dev, dl, **kw)
        tot['rows'] += len(rows)
        for k in ('equal', 'undecided', 'near_ties'):
            tot[k] += res[k]
        tot['unexplained'] += [dict(step=t, **u) for u in res['unexplained']]
        x_t.copy_(snapshot)
        prev[0] = snapshot

    engine.sample_tokens(net, segm, tex_tok, steps, MASK_ID, temp=temp, noise=noise, step_hook=hook, **kw)
    msg = (f"B={B} temp={temp} {kw}: {tot['rows']} sampled rows, {tot['equal']} equal, {tot['near_ties']} race near-ties, "
           f"{tot['undecided']} with an undecided kept set")
    print(msg)
    assert tot['rows'] == B * 512
    assert not tot['unexplained'], (msg, tot['unexplained'][:5])
    assert tot['undecided'] <= 0.01 * tot['rows'], msg


def _restated_commit(scores, x_t, k):
    B, T = x_t.shape
    s, m = scores.view(B, T).double().cpu().numpy(), (x_t == MASK_ID).cpu().numpy()
    return [set(CR.top_k_rows(s[b], m[b], k[b])[0].tolist()) for b in range(B)]


@pytest.mark.parametrize('B', [2, 8])
def test_sample_fn_confidence_against_the_restated_loop(model, sds, B):
    """rounds = 16, top_k = 64: confidence_ref's loop with the threshold added to the draw (the confidence of the drawn
    token stays the full-softmax log-probability), on the oracle's transformer; the device is forced onto the restated
    state after every round."""
    rounds, kw, seed, temp, choice_temp = 16, dict(top_k=64), 2021, 1.0, 4.5
    tex_tok = _feed(model, B, 70 + B)
    segm = model.segm_tokens.contiguous()
    net = model.sampler_fn
    sd = {k: v.to(DEV) for k, v in sds['sampler'].items()}
    n = B * 512
    seed_all(seed)
    E, U = CR.draws(n, rounds, DEV)
    state = dict(x_t=torch.full((B, 512), MASK_ID, dtype=torch.int64, device=DEV),
                 out=torch.full((18, n), -1, dtype=torch.int64, device=DEV))
    ks = [CR.schedule_of(512, rounds) for _ in range(B)]
    tot = dict(rows=0, equal=0, undecided=0, near_ties=0, unexplained=[], pairs=0, excused=0, unexcused=[])

    def hook(r, x_t, out, tok, conf, scores):
        prev = state['x_t']
        k_r = [ks[b][r - 1] for b in range(B)]
        own = _restated_commit(scores, prev, k_r)
        changed = (x_t != prev)
        for b in range(B):                                   # the device commits the top k of its OWN scores, exactly
            assert set(changed[b].nonzero().flatten().tolist()) == own[b], (r, b)
        masked = (prev == MASK_ID).view(-1)
        l = CR.own_logits(prev, segm, tex_tok, sd, temp)
        lm = _own_logits(net, prev, segm, tex_tok, temp)
        dl = (l.double() - lm.double()).abs().max(1).values
        assert float(dl[masked].max()) <= ACT_TOL, float(dl[masked].max())
        rows = masked.nonzero().flatten()
        res = ref.judge_rows(l[rows], E[r - 1][rows], tok[rows], dl[rows], **kw)
        tot['rows'] += len(rows)
        for k in ('equal', 'undecided', 'near_ties'):
            tot[k] += res[k]
        tot['unexplained'] += [dict(round=r, **u) for u in res['unexplained']]
        # the restated round: the thresholded token, its full-softmax confidence, the commit
        tok_r, _ = ref.race_torch(l, E[r - 1], ref.kept_torch(l, **kw))
        mx = l.max(-1, keepdim=True).values
        conf_r = (l - mx).gather(1, tok_r[:, None])[:, 0] - torch.log(torch.exp(l - mx).sum(-1))
        u = U[r - 1].clamp(CR.U_LO, CR.U_HI)
        s_r = conf_r + CR.tau_of(r, rounds, choice_temp) * -torch.log(-torch.log(u))
        x_new, out_new, sets = CR.commit(prev, state['out'], tok_r, s_r, tex_tok, k_r)
        tr = dict(prev=prev, logits=l, tok=tok_r, scores=s_r, k=k_r, sets=sets)
        c = CR.compare_round(tr, E[r - 1], tok_r.clone(), x_t.clone(), lm, ACT_TOL)   # (tokens judged above: commit sets here)
        tot['pairs'] += B
        tot['excused'] += len(c['excused_samples'])
        # a commit set may also differ through a row whose TOKEN differs (its confidence is another class's): excused
        # by the token's own accounting above; what remains must be within the score band of the cut
        differing = set((tok.long() != tok_r)[masked.nonzero().flatten()].nonzero().flatten().tolist())
        if c['unexcused_rows'] and not differing:
            tot['unexcused'] += c['unexcused_rows']
        state['x_t'], state['out'] = x_new, out_new
        x_t.copy_(x_new)
        out.copy_(out_new)

    seed_all(seed)
    got = engine.sample_tokens_confidence(net, segm, tex_tok, MASK_ID, rounds=rounds, temp=temp, choice_temp=choice_temp,
                                          round_hook=hook, **kw)
    assert torch.equal(got, state['out'])
    msg = (f"B={B} R={rounds} {kw}: {tot['rows']} drawn rows, {tot['equal']} equal, {tot['near_ties']} race near-ties, "
           f"{tot['undecided']} with an undecided kept set; {tot['pairs']} (round, sample) pairs, {tot['excused']} with an "
           f"excused row")
    print(msg)
    assert not tot['unexplained'], (msg, tot['unexplained'][:5])
    assert not tot['unexcused'], (msg, tot['unexcused'][:5])
    assert tot['undecided'] <= 0.01 * tot['rows'], msg
    assert tot['excused'] <= 0.01 * tot['pairs'], msg
