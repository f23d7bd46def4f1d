"""Float64 restatement of the all-codebook fit and the region vote: what t2h_vq_fit_books_f32 and
t2h_texture_vote are compared against, on the CPU and on the GPU (tests/test_vq_fit_emulated.py, tests/test_gpu_vq_fit.py).
Nothing here looks at what the kernels compute."""
import numpy as np

GROUPS = ((1, 4), (3, 5, 21), (2, ))  # upper, lower, outer: the classes of t2h_texture_map
NA = 17


def _dots(z, e):
    """[n, n_books, n_e] float64 dot products"""
    nb, n_e, d = e.shape
    return (z @ e.reshape(nb * n_e, d).T).reshape(z.shape[0], nb, n_e)


def fit_books64(z, books):
    """z [n, d], books [n_books, n_e, d] -> (d64 [n, n_books, n_e], its min [n, n_books], its first argmin)."""
    z = np.asarray(z, np.float64)
    e = np.asarray(books, np.float64)
    zz = (z * z).sum(1)
    ee = (e * e).sum(2)
    d64 = (zz[:, None, None] + ee[None]) - 2.0 * _dots(z, e)
    return d64, d64.min(2), d64.argmin(2)


def tol(z, books):
    """[n, n_books, n_e]: (256 + 4) 2^-24 (sum z^2 + sum e^2 + 2 sum |z_k e_k|) -- the worst-case rounding of three
    256-term fp32 accumulations in any order plus the final combination.  Derived, not measured."""
    z = np.abs(np.asarray(z, np.float64))
    e = np.abs(np.asarray(books, np.float64))
    zz = (z * z).sum(1)
    ee = (e * e).sum(2)
    return (256 + 4) * 2.0 ** -24 * ((zz[:, None, None] + ee[None]) + 2.0 * _dots(z, e))


def second_gap(d64):
    """[n, n_books]: float64 gap between the best and the second-best code"""
    part = np.partition(d64, 1, axis=2)
    return part[:, :, 1] - part[:, :, 0]


def check_fit(z, books, dmin, jmin, max_excused=0.01):
    """The kernel checks of the issue on one problem; -> the excused share of (row, book) pairs."""
    d64, m64, j64 = fit_books64(z, books)
    t = tol(z, books)
    n, nb, _ = d64.shape
    rr, hh = np.meshgrid(np.arange(n), np.arange(nb), indexing='ij')
    t_ref = t[rr, hh, j64]
    assert np.isfinite(dmin).all()
    assert (np.abs(dmin.astype(np.float64) - m64) <= t_ref).all(), float(np.abs(dmin - m64).max())
    if jmin is None:
        return 0.0
    assert ((jmin >= 0) & (jmin < d64.shape[2])).all()
    assert (d64[rr, hh, jmin] <= m64 + 2.0 * t_ref).all()
    decided = second_gap(d64) > 2.0 * t.max(2)   # (the reference alone decides who is excused)
    assert (jmin[decided] == j64[decided]).all()
    excused = 1.0 - decided.mean()
    assert excused <= max_excused, excused
    return excused


def in_group(lab, g):
    return np.isin(np.asarray(lab), GROUPS[g])


def vote(dmin, segm_tok):
    """dmin f32 [B*T, n_books], segm_tok [B, T] -> (cost f64 [B, 3, n_books], count i32 [B, 3], attr i64 [B, 3]):
    the ascending-row float64 sum and the decision rule (first least cost below +inf; book 0 and 'nothing' = 17)."""
    segm_tok = np.asarray(segm_tok)
    B, T = segm_tok.shape
    nb = dmin.shape[1]
    dm = np.asarray(dmin, np.float32).reshape(B, T, nb)
    cost = np.zeros((B, 3, nb), np.float64)
    count = np.zeros((B, 3), np.int32)
    attr = np.full((B, 3), NA, np.int64)
    with np.errstate(invalid='ignore'):
        for b in range(B):
            for g in range(3):
                rows = np.nonzero(in_group(segm_tok[b], g))[0]
                count[b, g] = rows.size
                for r in rows:                      # ascending rows, one float64 addition each
                    cost[b, g] += dm[b, r].astype(np.float64)
                best, bh = np.inf, -1
                if rows.size:
                    for h in range(nb):
                        if cost[b, g, h] < best:
                            best, bh = cost[b, g, h], h
                attr[b, g] = NA if bh <= 0 else bh - 1
    return cost, count, attr


def decide(cost, count):
    """the vote's decision rule on one region's costs [n_books] -> attribute"""
    best, bh = np.inf, -1
    if count:
        for h in range(cost.shape[0]):
            if cost[h] < best:
                best, bh = cost[h], h
    return NA if bh <= 0 else bh - 1


def region_costs64(z, books, segm_tok):
    """Everything in float64, from the latent rows: -> (cost64 [B, 3, n_books], tolsum [B, 3, n_books] = the summed
    per-row bound at the row's float64 argmin, count [B, 3], attr64 [B, 3], decided bool [B, 3] = the float64 gap
    between the least and the second least cost exceeds the summed 2 tol (of the worse of the books))."""
    segm_tok = np.asarray(segm_tok)
    B, T = segm_tok.shape
    _, m64, j64 = fit_books64(z, books)
    t_at = np.take_along_axis(tol(z, books), j64[:, :, None], 2)[:, :, 0]
    nb = m64.shape[1]
    m64, t_at = m64.reshape(B, T, nb), t_at.reshape(B, T, nb)
    cost = np.zeros((B, 3, nb))
    tolsum = np.zeros((B, 3, nb))
    count = np.zeros((B, 3), np.int32)
    attr = np.full((B, 3), NA, np.int64)
    decided = np.zeros((B, 3), bool)
    for b in range(B):
        for g in range(3):
            sel = in_group(segm_tok[b], g)
            count[b, g] = sel.sum()
            cost[b, g] = m64[b, sel].sum(0)
            tolsum[b, g] = t_at[b, sel].sum(0)
            attr[b, g] = decide(cost[b, g], count[b, g])
            if count[b, g]:
                two = np.sort(cost[b, g])[:2]
                decided[b, g] = two[1] - two[0] > 2.0 * tolsum[b, g].max()
            else:
                decided[b, g] = True   # nothing to sum: 17 whatever the arithmetic
    return cost, tolsum, count, attr, decided
