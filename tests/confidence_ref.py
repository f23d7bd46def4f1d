"""Plain torch restatement of confidence-ordered decoding ("Confidence-ordered decoding") on the oracle's
transformer (oracle/torch_ref.py), in the dtype of the state dict it is given -- shared by tests/test_gpu_confidence.py
and tools/confidence_parity_seeds.py.  Test infrastructure: the package never imports it."""
import math

import numpy as np
import torch

from oracle import torch_ref as R

MASK_ID, N_CLASS = 18432, 1024
U_LO, U_HI = 2.0**-24, 1.0 - 2.0**-24


def draws(n, rounds, device, n_class=N_CLASS):
    """The draws of a run, in the order the definition consumes the device generator: per round E then U."""
    E, U = [], []
    for _ in range(rounds):
        E.append(torch.empty(n, n_class, device=device).exponential_())
        U.append(torch.rand(n, device=device))
    return E, U


def own_logits(x_t, segm_tok, tex_tok, sd, temp):
    """[n, n_class] logits of every row's own texture head / temp, in sd's dtype"""
    tex = tex_tok.reshape(-1)
    n = tex.numel()
    present = set(tex.unique().tolist())
    with torch.no_grad():
        lg = R.transformer_logits(x_t, segm_tok, tex_tok, sd, heads=present)
    out = None
    for h in present:
        lh = lg[h].reshape(n, -1)
        if out is None:
            out = torch.zeros_like(lh)
        sel = tex == h
        out[sel] = lh[sel]
    return out / temp


def draw_and_score(l, E, U, tau):
    """-> (token [n], confidence [n], score [n]) of logits l [n, n_class] in l's dtype"""
    dt = l.dtype
    mx = l.max(-1, keepdim=True).values
    ex = torch.exp(l - mx)
    tok = torch.argmax(ex / E.to(dt), -1)                       # (first index of the maximum)
    conf = (l - mx).gather(1, tok[:, None])[:, 0] - torch.log(ex.sum(-1))
    u = U.to(dt).clamp(U_LO, U_HI)
    return tok, conf, conf + tau * -torch.log(-torch.log(u))


def top_k_rows(scores, masked, k):
    """rows (sorted by rank) of one sample: the k masked rows with the largest score, ties in row order, NaN last"""
    rows = np.nonzero(masked)[0]
    s = scores[rows].astype(np.float64)
    order = np.lexsort((rows, -np.where(np.isnan(s), -np.inf, s), np.isnan(s).astype(np.int64)))
    return rows[order][:max(int(k), 0)], rows[order]


def commit(x_t, out, tok, scores, tex_tok, ks):
    """in place on clones: x_t [B, T], out [18, B*T] -> (x_t, out, list of committed row arrays per sample)"""
    B, T = x_t.shape
    x_t, out = x_t.clone(), out.clone()
    tex = tex_tok.reshape(B, T)
    sets = []
    s_np, m_np = scores.reshape(B, T).double().cpu().numpy(), (x_t == MASK_ID).cpu().numpy()
    for b in range(B):
        rows, _ = top_k_rows(s_np[b], m_np[b], ks[b])
        sets.append(rows)
        if len(rows):
            r = torch.from_numpy(rows).to(x_t.device)
            tk = tok.reshape(B, T)[b, r].long()
            x_t[b, r] = tk + N_CLASS * tex[b, r]
            out[tex[b, r], b * T + r] = tk
    return x_t, out, sets


def tau_of(r, rounds, choice_temp):
    return float(np.float32(np.float64(choice_temp) * (1.0 - np.float64(r) / np.float64(rounds))))


def schedule_of(m0, rounds):
    """m_r / k_r written out from the definition (independent of text2human_amd.schedule)"""
    m = [int(m0)]
    for r in range(1, rounds + 1):
        v = 0 if r == rounds else math.floor(m0 * math.cos(math.pi / 2 * (r / rounds)))
        m.append(min(v, max(m[-1] - 1, 0)))
    return [m[i] - m[i + 1] for i in range(rounds)]


def run(segm_tok, tex_tok, sd, E, U, rounds, temp=1.0, choice_temp=4.5, x_t=None, out=None, trace=None):
    """The whole loop in sd's dtype -> (x_t, out); trace gets one dict per round."""
    B, T = tex_tok.shape
    dev = tex_tok.device
    if x_t is None:
        x_t = torch.full((B, T), MASK_ID, dtype=torch.int64, device=dev)
        out = torch.full((18, B * T), -1, dtype=torch.int64, device=dev)
    m0 = (x_t == MASK_ID).sum(1).tolist()
    ks = [schedule_of(m, rounds) for m in m0]
    for r in range(1, rounds + 1):
        k_r = [ks[b][r - 1] for b in range(B)]
        if (x_t == MASK_ID).sum() == 0:
            break
        l = own_logits(x_t, segm_tok, tex_tok, sd, temp)
        tok, conf, s = draw_and_score(l, E[r - 1], U[r - 1], tau_of(r, rounds, choice_temp))
        prev = x_t
        x_t, out, sets = commit(x_t, out, tok, s, tex_tok, k_r)
        if trace is not None:
            trace.append(dict(r=r, prev=prev, x_t=x_t, out=out, tok=tok, conf=conf, scores=s, logits=l, k=k_r, sets=sets))
    return x_t, out


def compare_round(tr, E, tok_other, x_after_other, logits_other, act_tol):
    """One teacher-forced round of another implementation (its tokens, its x_t after the round, its logits on the same
    input state) against the restated round `tr` (a trace dict of run()), by the rule of the parity tests:
    a drawn token that differs is explained iff the restatement's own score gap is <= 2 dl (dl = the row's largest logit
    difference between the two) and dl <= act_tol; a row that is committed by one side only is excused iff its restated
    score lies within 2 dl_max of the restated cut (midpoint of the k-th and (k+1)-th restated score).
    -> dict(token_mismatches, unexplained_tokens, excused_samples (list of b), unexcused_rows, dl_max)"""
    prev = tr['prev']
    B, T = prev.shape
    masked = (prev == MASK_ID).reshape(-1)
    lo = tr['logits'].double()
    dl = (lo - logits_other.double()).abs().max(-1).values
    dl_max = float(dl[masked].max()) if bool(masked.any()) else 0.0
    res = dict(token_mismatches=0, unexplained_tokens=[], excused_samples=[], unexcused_rows=[], dl_max=dl_max)
    diff = (masked & (tok_other.reshape(-1).long() != tr['tok'])).nonzero().flatten().tolist()
    res['token_mismatches'] = len(diff)
    for row in diff:
        score = torch.log_softmax(lo[row], -1) - E[row].double().log()
        gap = float(score[int(tr['tok'][row])] - score[int(tok_other.reshape(-1)[row])])
        if not (gap <= 2.0 * float(dl[row]) + 1e-7 and float(dl[row]) <= act_tol):
            res['unexplained_tokens'].append(dict(row=row, gap=gap, dl=float(dl[row])))
    s_np = tr['scores'].reshape(B, T).double().cpu().numpy()
    m_np = masked.reshape(B, T).cpu().numpy()
    changed = (x_after_other != prev).cpu().numpy()
    for b in range(B):
        theirs = set(np.nonzero(changed[b])[0].tolist())
        ours = set(tr['sets'][b].tolist())
        if theirs == ours:
            continue
        k = int(tr['k'][b])
        _, ranked = top_k_rows(s_np[b], m_np[b], k)
        if not 0 < k < len(ranked):
            res['unexcused_rows'].append(dict(sample=b, rows=sorted(theirs ^ ours), reason='no cut'))
            continue
        cut = 0.5 * (s_np[b][ranked[k - 1]] + s_np[b][ranked[k]])
        bad = [int(i) for i in sorted(theirs ^ ours) if not abs(s_np[b][i] - cut) <= 2.0 * dl_max + 1e-7]
        if bad or dl_max > act_tol:
            res['unexcused_rows'].append(dict(sample=b, rows=bad, cut=float(cut), dl_max=dl_max))
        else:
            res['excused_samples'].append(b)
    return res
