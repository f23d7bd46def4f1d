"""Truncated sampling (top-k / top-p) restated in numpy -- DESIGN.md, "Truncated sampling"; the contract the kernels of
csrc/sampler.hip compute.  Test infrastructure only.

For one row of temperature-scaled fp32 logits l:
  top-k   theta_k = the k-th largest value with multiplicity; l_j >= theta_k survives (ties at the threshold all do).
  top-p   on the survivors: m_j = floor(e_j 2^32) with e_j = expf(l_j - max l) in fp32, as 64-bit integers;
          S = sum of m over the survivors, G(v) = sum of m_i over survivors with l_i > v; j survives iff
          G(l_j) 2^20 < p_q S, p_q = rint(top_p 2^20).  theta_p = the smallest surviving value.
  theta = max(theta_k, theta_p); -0 and +0 are one value, reported as +0.

`kept_set` is that definition on integers, exactly, from a GIVEN array of fp32 exponentials (python integers: no
overflow, no summation order).  `top_p_sandwich` is an fp64, order-free oracle for the case where the kernel's own
exponentials are not available: a strict and a permissive set with p -+ d, d = 2^-18.  Where d comes from: two expf
implementations differ by a few ulp (<= 2^-21 relative per term), and flooring up to 1024 masses to multiples of 2^-32
loses <= 2^-22 of the largest mass, which is <= S; 2^-18 is an order of magnitude above the sum of the two.  It is a
bound on arithmetic, not a measured tolerance."""
import numpy as np

P_ONE = 1 << 20
D_BAND = 2.0**-18


def p_q_of(top_p):
    return int(np.rint(float(top_p) * P_ONE))


def canon(x):
    """-0 -> +0 (one value)"""
    return (np.asarray(x, dtype=np.float32) + np.float32(0.0)).astype(np.float32)


def masses(e32):
    """floor(e 2^32) of fp32 exponentials in [0, 1] as python integers (the scaling by 2^32 is exact in fp64)"""
    e = np.asarray(e32, dtype=np.float32).astype(np.float64)
    e = np.where(e >= 0.0, e, 0.0)                       # (NaN: no mass)
    return [int(v) for v in np.floor(e * 4294967296.0)]


def theta_k_of(l, top_k):
    l = np.asarray(l, dtype=np.float32)
    if not top_k or top_k >= l.size:
        return np.float32(-np.inf)
    return canon(np.sort(l)[::-1][top_k - 1])


def kept_set(l, e32=None, top_k=0, p_q=0):
    """-> (theta fp32, kept bool [n_class]) of one row; e32 (needed for top-p) = the fp32 values expf(l - max l)"""
    l = np.asarray(l, dtype=np.float32)
    theta = theta_k_of(l, top_k)
    keep = l >= theta
    if p_q and p_q != P_ONE:
        m = masses(e32)
        S = sum(m[j] for j in np.nonzero(keep)[0])
        theta_p = None
        G = 0
        vals = np.unique(l[keep])[::-1]                  # distinct surviving values, descending
        for v in vals:
            if G * P_ONE < p_q * S:
                theta_p = v
            else:
                break
            G += sum(m[j] for j in np.nonzero(keep & (l == v))[0])
        theta = canon(theta_p)
        keep = l >= theta
    return np.float32(theta), keep


def top_p_sandwich(l, p_q, survivors=None, d=D_BAND):
    """fp64, order-free: -> (strict, permissive) bool [n_class]: {j : G64(j) < (p -+ d) S64} among `survivors`
    (default: all classes), G64(j) = sum over survivors with l_i > l_j of exp(l_i - max l) (math.fsum: exactly
    rounded, no summation order)."""
    import math
    l = np.asarray(l, dtype=np.float32)
    surv = np.ones(l.shape, dtype=bool) if survivors is None else np.asarray(survivors, dtype=bool)
    l64 = l.astype(np.float64)
    e = np.exp(l64 - l64.max())
    S = math.fsum(e[surv])
    p = p_q / P_ONE
    order = np.argsort(-l64, kind='stable')
    strict, perm = np.zeros(l.shape, dtype=bool), np.zeros(l.shape, dtype=bool)
    i = 0
    above = []                                            # the exponentials of survivors strictly above the current value
    while i < l.size:
        v = l64[order[i]]
        j = i
        while j < l.size and l64[order[j]] == v:
            j += 1
        G = math.fsum(above)
        grp = order[i:j]
        grp = grp[surv[grp]]
        strict[grp] = G < (p - d) * S
        perm[grp] = G < (p + d) * S
        above.extend(e[grp].tolist())
        i = j
    return strict, perm


def race_winner(l, expo, keep):
    """argmax_j expf(l_j - max l) / E_j over the kept classes, first index wins (fp32 arithmetic; the exponentials are
    numpy's -- a test that needs the kernel's own scores compares tokens only where the margin is clear, or takes the
    kept set from the kernel)"""
    l = np.asarray(l, dtype=np.float32)
    sc = np.exp(l - l.max()).astype(np.float32) / np.asarray(expo, dtype=np.float32)
    sc = np.where(keep, sc, np.float32(-1.0))
    return int(np.argmax(sc))


# ---- the same definition on torch tensors (rows of a whole sampling round at once), in float64: the restatement the
# whole-loop GPU tests run next to the kernels.  Two implementations whose logits differ by up to dl per row cannot
# agree on a class whose logit lies within 2 dl of the threshold, nor on a top-p boundary within the change of the
# masses that dl causes (relative e^(2 dl) - 1 per mass, under 4 dl of the total for dl << 1) plus the integer band
# D_BAND; `slack` moves the threshold by exactly that much, to the strict (+1) or the permissive (-1) side.
def kept_torch(l, top_k=None, top_p=None, dl=None, slack=0):
    """l [n, n_class] (any float dtype) -> bool [n, n_class], the kept set; slack = +1 / -1: the strict / permissive
    set for a per-row logit uncertainty dl [n] (0: the definition itself)"""
    import torch
    l = l.double()
    n, c = l.shape
    dl = torch.zeros(n, dtype=torch.float64, device=l.device) if dl is None else dl.double()
    theta = torch.full((n, ), -float('inf'), dtype=torch.float64, device=l.device)
    if top_k and top_k < c:
        theta = l.topk(int(top_k), dim=1).values[:, -1]
    surv = l >= theta[:, None]
    if top_p is not None and top_p < 1.0:
        p = p_q_of(top_p) / P_ONE - slack * (D_BAND + 4.0 * dl)
        v, order = l.sort(dim=1, descending=True)
        e = torch.exp(v - v[:, :1]) * surv.gather(1, order)
        excl = e.cumsum(1) - e
        new = torch.ones_like(v, dtype=torch.bool)
        new[:, 1:] = v[:, 1:] != v[:, :-1]
        G = torch.where(new, excl, torch.zeros_like(excl)).cummax(1).values      # mass strictly above (ties share it)
        S = e.sum(1)
        ok = surv.gather(1, order) & (G < p[:, None] * S[:, None])
        ok[:, 0] = True                                                          # the most probable class: G = 0
        theta_p = torch.where(ok, v, torch.full_like(v, float('inf'))).min(1).values
        theta = torch.maximum(theta, theta_p)
    return l >= (theta + slack * 2.0 * dl)[:, None]


def race_torch(l, E, keep):
    """-> (token [n], log-score [n, n_class]) of the exponential race over the kept classes, float64, first index wins"""
    import torch
    score = torch.log_softmax(l.double(), 1) - E.double().log()
    return torch.where(keep, score, torch.full_like(score, -float('inf'))).argmax(1), score


def judge_rows(l, E, tok_dev, dl, top_k=None, top_p=None):
    """Device tokens tok_dev [n] against the restated draw on logits l that may differ from the device's by dl [n] per
    row -> dict(equal, undecided, near_ties, unexplained=[...]).  A row is `undecided` iff its strict and permissive
    kept sets have different winners (the kept set itself is inside the arithmetic band); otherwise a differing token
    must be a near-tie of the race: in the permissive set, and the restated log-score gap <= 2 dl."""
    import torch
    tok, score = race_torch(l, E, kept_torch(l, top_k, top_p))
    res = dict(equal=0, undecided=0, near_ties=0, unexplained=[])
    diff = (tok != tok_dev.long()).nonzero().flatten()
    res['equal'] = int(l.shape[0] - diff.numel())
    if diff.numel():
        ls, Es, dls = l[diff], E[diff], dl[diff]
        strict = kept_torch(ls, top_k, top_p, dls, +1)
        perm = kept_torch(ls, top_k, top_p, dls, -1)
        w_s, _ = race_torch(ls, Es, strict)
        w_p, sc = race_torch(ls, Es, perm)
        for i, row in enumerate(diff.tolist()):
            td = int(tok_dev[row])
            if int(w_s[i]) != int(w_p[i]):
                res['undecided'] += 1
                continue
            gap = float(sc[i, int(w_p[i])] - sc[i, td])
            if bool(perm[i, td]) and gap <= 2.0 * float(dls[i]) + 1e-7:
                res['near_ties'] += 1
            else:
                res['unexplained'].append(dict(row=row, device=td, restated=int(tok[row]), gap=gap, dl=float(dls[i]),
                                               in_permissive=bool(perm[i, td])))
    return res
