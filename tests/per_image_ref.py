"""Per-image sampling controls restated in numpy ("Per-image sampling controls"): the definitions of
tests/truncation_ref.py and tests/confidence_ref.py with the scalar replaced by the image's own value.  Row r of a
batch of B images with T rows each belongs to image r // T."""
import numpy as np

import confidence_ref as CR
import truncation_ref as TR


def settings(temp, top_k, top_p):
    """per-image (temp, top_k, top_p) of the public surface -> list of (temp, top_k, top_p_q), None = off"""
    return [(float(t), int(k or 0), TR.p_q_of(p) if p is not None else 0) for t, k, p in zip(temp, top_k, top_p)]


def table(sets):
    """list of (temp, top_k, top_p_q) -> the bytes of t2h_sample_params[B] as int32 [B, 3]"""
    out = np.zeros((len(sets), 3), dtype=np.int32)
    for b, (t, k, p_q) in enumerate(sets):
        out[b, 0] = np.float32(t).view(np.int32)
        out[b, 1], out[b, 2] = k, p_q
    return out


def top_k_thresholds(logits, sets, T):
    """theta [n] (fp32) and kept counts [n] of the top-k rule alone, row r under image r // T's top_k"""
    theta = np.empty(logits.shape[0], dtype=np.float32)
    kept = np.empty(logits.shape[0], dtype=np.int64)
    for r in range(logits.shape[0]):
        theta[r], keep = TR.kept_set(logits[r], top_k=sets[r // T][1])
        kept[r] = keep.sum()
    return theta, kept


def confidence_tables(m0, rounds, choice_temps):
    """-> (k int64 [R, B], tau float32 [R, B]), R = max rounds: column b = image b's own schedule / choice temperatures
    (confidence_ref.schedule_of / tau_of), zero after its last round"""
    R, B = max(rounds), len(m0)
    k, tau = np.zeros((R, B), dtype=np.int64), np.zeros((R, B), dtype=np.float32)
    for b in range(B):
        k[:rounds[b], b] = CR.schedule_of(m0[b], rounds[b])
        tau[:rounds[b], b] = [CR.tau_of(r, rounds[b], choice_temps[b]) for r in range(1, rounds[b] + 1)]
    return k, tau


def committed_rows(scores, masked, k):
    """per image: the set of its k[b] masked rows with the largest score (equal scores in row order, NaN last)"""
    return [set(CR.top_k_rows(scores[b], masked[b], k[b])[0].tolist()) for b in range(len(k))]
