"""Per-token log-probabilities of the index sampler restated in torch / numpy.

logp[row] = log_softmax(head_tex(LN_f(hidden[row])) / temp)[tok] -- the FULL softmax over all classes at the row's own
temperature, whatever truncation did to the draw.  `dtype` float64 is the reference; float32 is the same formula in
torch's own float32 arithmetic, whose distance from float64 is the yardstick of the kernels' error (f32_error)."""
import numpy as np
import torch
import torch.nn.functional as F

# max |float32 torch restatement - float64| of the log-probabilities of tests/test_logp_emulated.py's problem (C = 512,
# n_class = 1024, 18 heads) at its drawn tokens, per temperature, measured on the CPU with
#   f32_error(pb['hidden'], pb['gamma'], pb['beta'], pb['w'], pb['tex'], rows, tok, temp)
# (pb = that file's _problem(), rows / tok = the drawn rows and tokens of its `plain` fixture at that temperature).  A
# kernel may differ from float64 by 8 x that: the project's margin for another summation order over 512 + 1024 terms
# (tests/test_gpu_confidence.py).  The kernels themselves measured 8.3e-7 / 1.17e-6 / 5.9e-7 there.
LOGP_ERR_F32 = {1.0: 1.832e-6, 0.7: 2.087e-6, 1.3: 5.899e-7}


def row_logp(hidden, gamma, beta, w_heads, tex, rows, tok, temp, dtype=torch.float64):
    """hidden [n, C], w_heads [n_heads, n_class, C], tex int64 [n], rows = the drawn rows, tok[i] = the token of
    rows[i], temp a scalar or one value per listed row -> numpy float64 [len(rows)] (computed in `dtype`)"""
    rows = torch.as_tensor(np.asarray(rows), dtype=torch.int64)
    tok = torch.as_tensor(np.asarray(tok), dtype=torch.int64)
    temp = torch.as_tensor(np.broadcast_to(np.asarray(temp, dtype=np.float64), (len(rows), )).copy()).to(dtype)
    y = F.layer_norm(hidden[rows].to(dtype), (hidden.shape[1], ), gamma.to(dtype), beta.to(dtype), 1e-5)
    logits = torch.einsum('rc,rkc->rk', y, w_heads[tex[rows]].to(dtype)) / temp[:, None]
    lp = torch.log_softmax(logits, -1)
    return lp.gather(1, tok[:, None])[:, 0].double().numpy()


def f32_error(hidden, gamma, beta, w_heads, tex, rows, tok, temp):
    """max |float32 restatement - float64| over the rows: what float32 arithmetic costs on these very inputs"""
    args = (hidden, gamma, beta, w_heads, tex, rows, tok, temp)
    return float(np.abs(row_logp(*args, dtype=torch.float32) - row_logp(*args)).max())


def logits_logp(logits, tok):
    """float64 log-softmax of kernel-made logits (already divided by the temperature) at tok: [rows, n_class] -> [rows]"""
    l = np.asarray(logits, dtype=np.float64)
    m = l.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(l - m).sum(1))
    return l[np.arange(l.shape[0]), np.asarray(tok)] - lse


def summary(logp):
    """logp [B, T] with NaN = never drawn -> (sum float64 [B], count int64 [B], min float32 [B], abs-sum float64 [B])"""
    v = np.asarray(logp, dtype=np.float32)
    ok = ~np.isnan(v)
    d = np.where(ok, v.astype(np.float64), 0.0)
    mn = np.where(ok, v, np.float32(np.inf)).min(1).astype(np.float32)
    return d.sum(1), ok.sum(1).astype(np.int64), mn, np.abs(d).sum(1)


def best_of(logps):
    """logps [n_candidates, B, T] -> (choice int64 [B], score float64 [B]): per image the candidate with the highest mean
    log-probability per drawn token (no drawn token: -inf), the earlier candidate on a tie"""
    scores = []
    for lp in logps:
        s, c, _, _ = summary(lp)
        scores.append(np.where(c > 0, s / np.maximum(c, 1), -np.inf))
    scores = np.stack(scores)
    choice = scores.argmax(0)  # (the first maximum)
    return choice.astype(np.int64), scores.max(0)
