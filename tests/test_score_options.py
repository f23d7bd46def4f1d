"""Scoring a given token map: the surface without a GPU -- the graph keys of every call that does not
score are the tuples they were, a scoring key differs by its one trailing element, the C-ABI mirror, and score_fn's
argument validation before anything is evaluated or drawn."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from text2human_amd import _lib, engine, ops
from text2human_amd.models.sample_model import BaseSampleModel

import score_ref as ref  # noqa: E402

BASE = dict(B=8, T=512, sample_steps=256, maxr=64, temp=1.0, mask_id=18432, n_books=18, x8=True)
PER = dict(B=8, T=512, sample_steps=256, maxr=64, mask_id=18432, n_books=18, x8=True)


def test_graph_keys_of_calls_that_do_not_score_are_unchanged_tuples():
    plain = engine.round_graph_key(**BASE)
    assert plain == (8, 512, 256, 64, 1.0, 18432, 18, True, 0, 0)
    assert engine.round_graph_key(**BASE, score=None) == plain
    assert engine.round_graph_key(**BASE, logp=True) == plain + ('logp', )
    assert engine.round_graph_key(**BASE, trunc=(64, 0)) == (8, 512, 256, 64, 1.0, 18432, 18, True, 64, 0)
    per = engine.round_graph_key_per_image(**PER)
    assert per == (8, 512, 256, 64, 18432, 18, True, 'per-sample')
    assert engine.round_graph_key_per_image(**PER, score=None) == per
    assert engine.round_graph_key_per_image(**PER, logp=True) == per + ('logp', )
    for fn in (engine.round_graph_key, engine.round_graph_key_per_image):
        assert inspect.signature(fn).parameters['score'].default is None
    assert inspect.signature(engine.RoundGraph.__init__).parameters['score'].default is None
    assert inspect.signature(engine.RoundGraph.run).parameters['targets'].default is None
    for fn, names in ((engine._round, ('targets', 'rank')), (ops.sample_heads, ('targets', 'rank'))):
        for name in names:
            assert inspect.signature(fn).parameters[name].default is None, (fn, name)


def test_a_scoring_key_differs_only_by_its_trailing_element():
    plain, per = engine.round_graph_key(**BASE), engine.round_graph_key_per_image(**PER)
    kinds = (engine.SCORE, engine.SCORE_RANK)
    assert len(set(kinds)) == 2 and all(isinstance(k, str) and k != 'logp' for k in kinds)
    for kind in kinds:
        assert engine.round_graph_key(**BASE, score=kind) == plain + (kind, )
        assert engine.round_graph_key_per_image(**PER, score=kind) == per + (kind, )
    # the temperature is still held by value in the scalar key, and by no value in the per-image one
    assert engine.round_graph_key(**dict(BASE, temp=0.7), score=engine.SCORE)[:-1] == engine.round_graph_key(**dict(BASE, temp=0.7))


def test_the_c_abi_mirror():
    assert [f[0] for f in _lib.ScoreOut._fields_] == ['targets', 'rank']
    assert ctypes.sizeof(_lib.ScoreOut) == 2 * ctypes.sizeof(ctypes.c_void_p)
    s = _lib.ScoreOut()
    assert s.targets is None and s.rank is None                                  # zero-initialised: no rank output
    head, out = ctypes.POINTER(_lib.SampleHeadsArgs), ctypes.POINTER(_lib.ScoreOut)
    assert _lib.SIGNATURES['t2h_score_heads'] == (ctypes.c_int, [head, out, ctypes.c_void_p])
    assert _lib.SIGNATURES['t2h_score_heads_per_sample'] == (ctypes.c_int, [head, out, ctypes.c_void_p, ctypes.c_int32,
                                                                           ctypes.c_void_p])
    assert _lib.SampleHeadsArgs._fields_[-1][0] == 'logp'                        # the sampling struct got no new field


def test_score_tokens_and_score_fn_signatures():
    p = inspect.signature(engine.score_tokens).parameters
    assert list(p) == ['net', 'segm_tok', 'tex_tok', 'sample_steps', 'mask_id', 'targets', 'temp', 'noise', 'n_books',
                       'keep', 'compact', 'round_hook', 'return_rank']
    assert p['temp'].default == 1.0 and p['n_books'].default == 18 and p['return_rank'].default is False
    assert 'top_k' not in p and 'top_p' not in p
    q = inspect.signature(BaseSampleModel.score_fn).parameters
    assert list(q) == ['self', 'top_indices_list', 'keep', 'temp', 'sample_steps', 'return_rank', 'summary']
    assert q['keep'].default is None and q['temp'].default == 1.0 and q['summary'].default is False


def _model(batch=2):
    m = BaseSampleModel.__new__(BaseSampleModel)                                 # (no device: nothing may be touched)
    m.batch_size, m.shape, m.sample_steps, m.device = batch, (32, 16), 256, torch.device('cpu')
    return m


def test_score_fn_validates_before_anything_is_evaluated_or_drawn():
    m = _model()
    good = [torch.zeros(2, 512, dtype=torch.int64) for _ in range(18)]
    state = torch.get_rng_state()
    for bad in (0, 0.0, -1.0, float('inf'), float('nan'), True, None, '1'):
        with pytest.raises(ValueError, match='temp'):
            m.score_fn(good, temp=bad)
    with pytest.raises(ValueError, match='temp'):
        m.score_fn(good, temp=[1.0, 0.0])                                        # per image: every entry
    with pytest.raises(ValueError, match='temp'):
        m.score_fn(good, temp=[1.0, 1.0, 1.0])                                   # ... and one entry per image
    for bad in (good[:17], [torch.zeros(2, 511, dtype=torch.int64) for _ in range(18)], torch.zeros(18, 3 * 512)):
        with pytest.raises(ValueError, match='score_fn: 18 index lists'):
            m.score_fn(bad)
    for bad in (torch.zeros(2, 511, dtype=torch.uint8), torch.zeros(1024, dtype=torch.uint8),
                torch.zeros(3, 512, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='keep must be'):
            m.score_fn(good, keep=bad)
    assert torch.equal(torch.get_rng_state(), state)


def test_score_tokens_rejects_a_map_of_another_shape():
    segm = torch.zeros(2, 512, dtype=torch.int64)
    for bad in (torch.zeros(18, 1023, dtype=torch.int64), torch.zeros(17, 1024, dtype=torch.int64),
                torch.zeros(18, 1024, dtype=torch.int32)):
        with pytest.raises(ValueError, match='targets'):
            engine.score_tokens(None, segm, segm, 16, 18432, bad)


def test_reference_rank_counts_strictly_greater():
    lg = np.array([[0.5, 2.0, 2.0, -1.0], [3.0, 3.0, 3.0, 3.0]], dtype=np.float32)
    assert ref.rank(lg, [1, 0]).tolist() == [0, 0]                               # a tied mode is a mode
    assert ref.rank(lg, [0, 3]).tolist() == [2, 0] and ref.rank(lg, [3, 1]).tolist() == [3, 0]
