"""Scoring a given token map restated in float64.

The log-probability of a target is logp_ref.row_logp at that target: the definition does not care whether the token
was drawn or handed in.  rank is defined on the kernel's OWN float32 logits -- it is a count of exact comparisons, so a
reference that recomputed the logits in another precision could disagree about near-ties without either being wrong."""
import numpy as np

from logp_ref import f32_error, logits_logp, row_logp  # noqa: F401  (the value reference, re-exported)


def rank(logits, tok):
    """logits [rows, n_class] as the logits kernel wrote them (already divided by the temperature), tok [rows] ->
    int64 [rows]: the number of classes with a STRICTLY greater logit than the target's (0 = the mode, or one of
    several tied modes)"""
    lg = np.asarray(logits, dtype=np.float32)
    tok = np.asarray(tok, dtype=np.int64)
    return (lg > lg[np.arange(lg.shape[0]), tok][:, None]).sum(1).astype(np.int64)
