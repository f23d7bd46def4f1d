"""Self-correction: the surface without a GPU -- the option keys and command-line flags, the row
counts of a pass, the batching rule of the critic, and the argument validation of pll_fn / revise_fn before anything is
evaluated or drawn."""
import inspect

import pytest
import torch

from text2human_amd import defaults, options, sample_from_parsing
from text2human_amd.models.sample_model import BaseSampleModel

import revise_ref as ref  # noqa: E402


def test_absent_keys_and_zero_passes_are_off_and_change_nothing():
    opt = defaults.sample_from_parsing()
    before = dict(opt)
    assert options.revise_settings(opt) is None and dict(opt) == before
    opt['revise_passes'] = 0
    assert options.revise_settings(opt) is None
    assert {k: v for k, v in opt.items() if k != 'revise_passes'} == before       # the existing keys are as they were
    assert list(opt)[:len(before)] == list(before)
    assert options.revise_settings(options.dict_to_nonedict(dict(opt))) is None


def test_defaults_and_given_values_parse():
    opt = defaults.with_revision(defaults.sample_from_parsing(), passes=2)
    assert options.revise_settings(opt) == (2, 0.25, 4)
    opt = defaults.with_revision(defaults.sample_from_parsing(), passes=1, fraction=0.5, folds=8)
    assert options.revise_settings(opt) == (1, 0.5, 8)
    assert options.revise_settings(defaults.with_revision(opt, passes=0)) is None and 'revise_folds' not in opt
    assert options.revise_settings(dict(revise_passes=3, revise_fraction=1, revise_folds=16)) == (3, 1.0, 16)
    assert options.REVISE_FOLDS == ref.FOLDS


@pytest.mark.parametrize('key,bad', [('revise_passes', -1), ('revise_passes', 1.5), ('revise_passes', True),
                                     ('revise_passes', '2'), ('revise_fraction', 0), ('revise_fraction', 0.0),
                                     ('revise_fraction', 1.0001), ('revise_fraction', -0.25), ('revise_fraction', 'x'),
                                     ('revise_fraction', float('nan')), ('revise_fraction', [0.25, 0.5]),
                                     ('revise_fraction', True), ('revise_folds', 3), ('revise_folds', 0),
                                     ('revise_folds', 32), ('revise_folds', 4.5), ('revise_folds', True)])
def test_bad_option_values_raise(key, bad):
    for passes in (1, 0):                                                        # validated whether the feature is on or not
        opt = dict(revise_passes=passes)
        opt[key] = bad
        with pytest.raises(ValueError, match=key.replace('revise_', '')):
            options.revise_settings(opt)


def test_cli_flags_set_the_keys_and_are_validated():
    ap = sample_from_parsing.cli_parser()
    ns = ap.parse_args(['-opt', 'x.yml', '--revise-passes', '2', '--revise-fraction', '0.1', '--revise-folds', '8'])
    opt = sample_from_parsing.apply_cli(defaults.sample_from_parsing(), ns)
    assert (opt['revise_passes'], opt['revise_fraction'], opt['revise_folds']) == (2, 0.1, 8)
    assert options.revise_settings(opt) == (2, 0.1, 8)
    plain = sample_from_parsing.apply_cli(defaults.sample_from_parsing(), ap.parse_args(['-opt', 'x.yml']))
    assert not any(k.startswith('revise_') for k in plain) and dict(plain) == dict(defaults.sample_from_parsing())
    with pytest.raises(ValueError, match='fraction'):
        sample_from_parsing.apply_cli(defaults.sample_from_parsing(),
                                      ap.parse_args(['-opt', 'x.yml', '--revise-passes', '1', '--revise-fraction', '1.5']))
    with pytest.raises(ValueError, match='passes'):
        sample_from_parsing.apply_cli(defaults.sample_from_parsing(), ap.parse_args(['-opt', 'x.yml', '--revise-passes', '-2']))
    with pytest.raises(SystemExit):
        ap.parse_args(['-opt', 'x.yml', '--revise-folds', '3'])


def test_row_counts_of_a_pass():
    elig = [512, 256, 3, 1, 0, 2]
    assert options.revise_row_counts(elig, fraction=0.25) == [128, 64, 1, 1, 0, 1] == ref.row_counts(elig, fraction=0.25)
    assert options.revise_row_counts(elig, fraction=1.0) == [512, 256, 3, 1, 0, 2]
    assert options.revise_row_counts([512], fraction=0.001) == [1]                # at least one row where any is eligible
    assert options.revise_row_counts([5, 5], fraction=[0.5, 0.3]) == [3, 2]       # 2.5 + 0.5 -> 3, 1.5 + 0.5 -> 2
    for f in (0.01, 0.1, 0.3, 0.33, 0.5, 0.9):
        assert options.revise_row_counts(elig, fraction=f) == ref.row_counts(elig, fraction=f)
    assert options.revise_row_counts(elig, count=3) == [3, 3, 3, 1, 0, 2] == ref.row_counts(elig, count=3)
    assert options.revise_row_counts([512, 512, 256], count=[3, 0, 512]) == [3, 0, 256]
    for kw in (dict(fraction=0.25, count=1), dict()):
        with pytest.raises(ValueError, match='either fraction or count'):
            options.revise_row_counts(elig, **kw)
    for bad in (0, 1.5, -1, True, None, '0.5', float('nan'), [0.5] * 5, [0.5] * 5 + [0.0]):
        with pytest.raises(ValueError):
            options.revise_row_counts(elig, fraction=bad) if bad is not None else options.revise_fractions(6, bad)
    for bad in (-1, 1.0, True, '3', [1] * 5, [1] * 5 + [-1], 1 << 31):
        with pytest.raises(ValueError, match='count'):
            options.revise_row_counts(elig, count=bad)


def test_the_batching_rule_depends_on_batch_and_folds_alone():
    assert inspect.signature(options.pll_batched).parameters.keys() == {'batch', 'folds'}
    assert options.PLL_BATCH_MAX == 32
    for b, k, want in ((1, 4, True), (1, 16, True), (8, 4, True), (3, 4, True), (3, 2, True), (8, 8, False),
                       (9, 4, False), (32, 2, False), (2, 16, True), (3, 16, False)):
        assert options.pll_batched(b, k) is want, (b, k)


def test_signatures():
    p = inspect.signature(BaseSampleModel.pll_fn).parameters
    assert list(p) == ['self', 'top_indices_list', 'keep', 'folds', 'temp', 'return_rank', 'summary']
    assert (p['keep'].default, p['folds'].default, p['temp'].default) == (None, 4, 1.0)
    assert p['return_rank'].default is False and p['summary'].default is False
    q = inspect.signature(BaseSampleModel.revise_fn).parameters
    assert list(q) == ['self', 'top_indices_list', 'passes', 'fraction', 'count', 'keep', 'folds', 'accept', 'temp',
                       'critic_temp', 'sample_steps', 'order', 'rounds', 'choice_temp', 'top_k', 'top_p', 'seeds',
                       'return_trace']
    want = dict(passes=1, fraction=0.25, count=None, keep=None, folds=4, accept='improve', temp=1.0, critic_temp=1.0,
                sample_steps=None, order='random', rounds=None, choice_temp=4.5, top_k=None, top_p=None, seeds=None,
                return_trace=False)
    assert {k: q[k].default for k in want} == want
    # the entry points that exist keep their parameter lists
    assert list(inspect.signature(BaseSampleModel.sample_and_refine).parameters) == ['self', 'save_dir', 'img_name', 'seeds']
    assert list(inspect.signature(BaseSampleModel.score_fn).parameters) == ['self', 'top_indices_list', 'keep', 'temp',
                                                                          'sample_steps', 'return_rank', 'summary']


def _model(batch=2):
    m = BaseSampleModel.__new__(BaseSampleModel)                                 # (no device: nothing may be touched)
    m.batch_size, m.shape, m.sample_steps, m.device = batch, (32, 16), 256, torch.device('cpu')
    return m


GOOD = [torch.zeros(2, 512, dtype=torch.int64) for _ in range(18)]


def test_pll_fn_validates_before_anything_is_evaluated():
    m = _model()
    state = torch.get_rng_state()
    for bad in (0, 1, 3, 5, 32, 4.5, True, None, '4'):
        with pytest.raises(ValueError, match='folds'):
            m.pll_fn(GOOD, folds=bad)
    for bad in (0, -1.0, float('inf'), float('nan'), True, None, [1.0, 0.0], [1.0] * 3):
        with pytest.raises(ValueError, match='temp'):
            m.pll_fn(GOOD, temp=bad)
    with pytest.raises(ValueError, match='pll_fn: 18 index lists'):
        m.pll_fn(GOOD[:17])
    with pytest.raises(ValueError, match='keep must be'):
        m.pll_fn(GOOD, keep=torch.zeros(2, 511, dtype=torch.uint8))
    assert torch.equal(torch.get_rng_state(), state)


def test_revise_fn_validates_before_anything_is_evaluated_or_drawn():
    m = _model()
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match='either fraction or count'):
        m.revise_fn(GOOD, fraction=0.5, count=3)
    with pytest.raises(ValueError, match='either fraction or count'):
        m.revise_fn(GOOD, fraction=0.25, count=3)                                # (also when the fraction given is the default's)
    for bad in (0, 0.0, 1.5, -0.1, True, None, 'x', [0.5], [0.5, 0.0]):
        with pytest.raises(ValueError, match='fraction'):
            m.revise_fn(GOOD, fraction=bad)
    for bad in (-1, 2.0, True, [1], [1, -1], '1'):
        with pytest.raises(ValueError, match='count'):
            m.revise_fn(GOOD, count=bad)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match='passes'):
            m.revise_fn(GOOD, passes=bad)
    for bad in (3, 0, None):
        with pytest.raises(ValueError, match='folds'):
            m.revise_fn(GOOD, folds=bad)
    for bad in ('never', None, True):
        with pytest.raises(ValueError, match='accept'):
            m.revise_fn(GOOD, accept=bad)
    for bad in (0, float('nan'), [1.0] * 3):
        with pytest.raises(ValueError, match='temp'):
            m.revise_fn(GOOD, critic_temp=bad)
    with pytest.raises(ValueError, match='order'):
        m.revise_fn(GOOD, order='raster')
    with pytest.raises(ValueError, match='per-image seeds are not supported'):
        m.revise_fn(GOOD, order='confidence', seeds=[1, 2])
    for bad in ([1], [1, -1], [1, 1 << 64], 5):
        with pytest.raises(ValueError, match='seeds'):
            m.revise_fn(GOOD, seeds=bad)
    with pytest.raises(ValueError, match='top_p'):
        m.revise_fn(GOOD, top_p=1.5)
    with pytest.raises(ValueError, match='keep must be'):
        m.revise_fn(GOOD, keep=torch.zeros(2, 511, dtype=torch.uint8))
    with pytest.raises(ValueError, match='revise_fn: 18 index lists'):
        m.revise_fn(GOOD[:17])
    assert torch.equal(torch.get_rng_state(), state)
