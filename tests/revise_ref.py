"""Self-correction restated in numpy: the fold lattice of the pseudo-likelihood critic, the choice of
the rows a pass redoes, the number of those rows and the accept rule.  Written from the definitions, not from the
kernels: plain loops and Python's own float comparisons."""
import math

import numpy as np

FOLDS = (2, 4, 8, 16)


def fold_of(i, tw, K):
    """the fold of token row i of a map with tw columns"""
    r, c = divmod(int(i), int(tw))
    if K == 2:
        return (r + c) % 2
    if K == 4:
        return (r % 2) * 2 + c % 2
    if K == 8:
        return (r % 4) * 2 + c % 2
    if K == 16:
        return (r % 4) * 4 + c % 4
    raise ValueError(f'folds must be one of {FOLDS}, got {K!r}')


def fold_map(th, tw, K):
    """int64 [th * tw]: the fold of every row"""
    return np.array([fold_of(i, tw, K) for i in range(th * tw)], dtype=np.int64)


def fold_keep(K, B, th, tw, keep=None):
    """uint8 [K, B, th * tw]: 1 iff the row is not in fold k or the caller keeps it (keep: [B, th * tw] or None)"""
    f = fold_map(th, tw, K)
    out = np.ones((K, B, th * tw), dtype=np.uint8)
    for k in range(K):
        for b in range(B):
            for i in range(th * tw):
                kept = keep is not None and keep[b][i] != 0
                out[k, b, i] = 0 if (f[i] == k and not kept) else 1
    return out


def neighbours(i, th, tw):
    """the up to eight neighbours of row i"""
    r, c = divmod(i, tw)
    return [rr * tw + cc for rr in (r - 1, r, r + 1) for cc in (c - 1, c, c + 1)
            if (rr, cc) != (r, c) and 0 <= rr < th and 0 <= cc < tw]


def select_lowest(score, count):
    """score float32 [B, T] (NaN = not eligible), count [B] -> (keep_out uint8 [B, T], n_sel int32 [B]): the
    min(max(count, 0), eligible) rows that come first in the order (value ascending by < / ==, then row index) are 0"""
    score = np.asarray(score, dtype=np.float32)
    B, T = score.shape
    keep_out = np.ones((B, T), dtype=np.uint8)
    n_sel = np.zeros(B, dtype=np.int32)
    for b in range(B):
        rows = [i for i in range(T) if not math.isnan(float(score[b, i]))]
        # an insertion sort on the two comparisons the definition names (no sort key: -0.0 == +0.0 must tie)
        order = []
        for i in rows:
            v = float(score[b, i])
            at = len(order)
            for pos, j in enumerate(order):
                w = float(score[b, j])
                if v < w or (v == w and i < j):
                    at = pos
                    break
            order.insert(at, i)
        m = min(max(int(count[b]), 0), len(rows))
        keep_out[b, order[:m]] = 0
        n_sel[b] = m
    return keep_out, n_sel


def row_counts(eligible, fraction=None, count=None):
    """rows a pass redoes per image: min(count, eligible), else max(1, floor(fraction * eligible + 0.5)) in float64 (0
    where nothing is eligible); fraction / count a scalar or one per image"""
    B = len(eligible)
    per = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * B
    if count is not None:
        return [min(int(c), int(e)) for c, e in zip(per(count), eligible)]
    return [0 if int(e) == 0 else max(1, int(math.floor(np.float64(f) * np.float64(int(e)) + np.float64(0.5))))
            for f, e in zip(per(fraction), eligible)]


def accept(sum_cand, sum_cur, mode):
    """bool [B]: the images that take the candidate"""
    if mode == 'always':
        return np.ones(len(sum_cur), dtype=bool)
    return np.array([float(c) > float(u) for c, u in zip(sum_cand, sum_cur)], dtype=bool)
