"""Confidence-ordered decoding, host side ("Confidence-ordered decoding"): the cosine schedule
(schedule.confidence_schedule: rows still masked after / committed in every round), the choice temperatures, and the
option keys that switch the mode on (absent keys leave the model on the reference's loop)."""
import math
import os

import numpy as np
import pytest

from text2human_amd import defaults, options, schedule

ROUNDS = [1, 2, 8, 16, 64, 512, 600]
M0S = [0, 1, 7, 100, 512]


@pytest.mark.parametrize('R', ROUNDS)
@pytest.mark.parametrize('m0', M0S)
def test_schedule_is_the_forced_cosine(R, m0):
    m, k = schedule.confidence_schedule(m0, R)
    assert m.shape == (R + 1, ) and k.shape == (R, )
    assert m[0] == m0 and m[R] == 0
    assert (np.diff(m) <= 0).all() and (k >= 0).all()          # non-increasing
    assert int(k.sum()) == m0
    assert (k[m[:-1] > 0] >= 1).all()                            # a round commits while anything is masked
    assert (k[m[:-1] == 0] == 0).all()
    for r in range(1, R + 1):
        raw = math.floor(m0 * math.cos(math.pi / 2 * (r / R)))
        cap = max(int(m[r - 1]) - 1, 0)
        if r < R and raw <= cap:                                 # neither forcing rule bites: the formula itself
            assert m[r] == raw, (r, m[r], raw)
        else:
            assert m[r] == (0 if r == R else cap)


def test_schedule_examples():
    m, k = schedule.confidence_schedule(512, 1)
    assert m.tolist() == [512, 0] and k.tolist() == [512]
    m, k = schedule.confidence_schedule(512, 2)
    assert m.tolist() == [512, math.floor(512 * math.cos(math.pi / 4)), 0]
    m, k = schedule.confidence_schedule(512, 512)
    assert (k == 1).all()                                        # one row per round
    m, k = schedule.confidence_schedule(512, 600)
    assert (k[:512] == 1).all() and (k[512:] == 0).all()
    m, k = schedule.confidence_schedule(7, 16)
    assert k.sum() == 7 and (k[:7] == 1).all()                   # the cosine would hold 6 rows for several rounds
    with pytest.raises(ValueError):
        schedule.confidence_schedule(512, 0)


def test_choice_temperatures():
    t = schedule.confidence_choice_temps(16, 4.5)
    assert t.dtype == np.float32 and t.shape == (16, )
    assert t[-1] == 0.0 and np.allclose(t, 4.5 * (1 - np.arange(1, 17) / 16), rtol=1e-7)
    assert (schedule.confidence_choice_temps(8, 0.0) == 0).all()


def test_option_keys_parse(tmp_path):
    opt = defaults.sample_from_parsing()
    assert options.sampling_order(opt) is None                   # absent keys: the reference's loop
    assert 'sample_order' not in opt
    path = defaults.write_yaml(defaults.with_confidence_order(defaults.sample_from_parsing(), rounds=8, choice_temp=2.0),
                               str(tmp_path / 'c.yml'))
    parsed = options.dict_to_nonedict(options.parse(path, root=str(tmp_path)))
    assert parsed['sample_order'] == 'confidence' and parsed['confidence_rounds'] == 8
    assert options.sampling_order(parsed) == (8, 2.0)
    # defaults of the two numeric keys; `random` is the old path
    assert options.sampling_order(options.dict_to_nonedict({'sample_order': 'confidence'})) == (16, 4.5)
    assert options.sampling_order(options.dict_to_nonedict({'sample_order': 'random', 'confidence_rounds': 8})) is None
    assert options.sampling_order(options.dict_to_nonedict({'confidence_rounds': 8})) is None
    for bad in ({'sample_order': 'best'}, {'sample_order': 'confidence', 'confidence_rounds': 0},
                {'sample_order': 'confidence', 'confidence_choice_temp': -1.0}):
        with pytest.raises(ValueError):
            options.sampling_order(options.dict_to_nonedict(bad))


def test_model_reads_the_mode_from_the_options_only():
    """sample_and_refine takes the new path iff options.sampling_order says so (source-level: no GPU here)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'text2human_amd', 'models',
                            'sample_model.py')).read()
    body = src[src.index('def sample_and_refine'):src.index('def inference')]
    assert 'self._confidence_options()' in body and 'self.sample_fn(temp=1, sample_steps=self.sample_steps)' in body
    assert 'return options.sampling_order(self.opt)' in src
