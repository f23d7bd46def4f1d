"""Host-side logic of garment colour control, no GPU: the options and their validation, the command
line, and that without a `recolor_*` key sample_and_refine does not enter the new code (the two ops are patched to
raise)."""
import pytest
import torch

from text2human_amd import defaults, ops, options, sample_from_parsing
from text2human_amd.models import sample_model

KEYS = ('recolor_upper', 'recolor_lower', 'recolor_outer', 'recolor_feather', 'recolor_luma')


def test_absent_means_off_and_nothing_is_added():
    opt = defaults.sample_from_parsing()
    before = dict(opt)
    assert options.recolor_settings(opt) is None and dict(opt) == before
    assert not any(k in opt for k in KEYS)
    assert options.recolor_settings(options.dict_to_nonedict(dict(opt))) is None
    assert options.recolor_settings(dict(recolor_feather=3, recolor_luma=0.5)) is None     # (no colour: still off)


def test_keys_and_defaults():
    opt = defaults.with_recolor(defaults.sample_from_parsing(), upper=(0.8, 0.1, 0.1))
    assert opt['recolor_upper'] == [0.8, 0.1, 0.1] and 'recolor_feather' not in opt
    assert options.recolor_settings(opt) == ({'upper': (0.8, 0.1, 0.1)}, 2, 1.0)
    defaults.with_recolor(opt, lower=[0, 0, 1], outer=(1, 1, 1), feather=0, luma=0.25)
    assert options.recolor_settings(opt) == ({'lower': (0.0, 0.0, 1.0), 'outer': (1.0, 1.0, 1.0)}, 0, 0.25)
    assert options.recolor_settings(defaults.with_recolor(opt)) is None and not any(k in opt for k in KEYS)
    assert options.recolor_settings(dict(recolor_outer=[0.5, 0.5, 0.5], recolor_feather=8)) == \
        ({'outer': (0.5, 0.5, 0.5)}, 8, 1.0)


@pytest.mark.parametrize('key,bad', [('recolor_upper', [0.5, 0.5]), ('recolor_upper', [0.5, 0.5, 1.5]),
                                     ('recolor_lower', [-0.1, 0, 0]), ('recolor_lower', 'red'), ('recolor_outer', 0.5),
                                     ('recolor_outer', [0.1, 0.2, 'x']), ('recolor_outer', [0.1, 0.2, float('nan')]),
                                     ('recolor_upper', [True, 0, 0]), ('recolor_feather', -1), ('recolor_feather', 9),
                                     ('recolor_feather', 2.5), ('recolor_feather', True), ('recolor_luma', -0.1),
                                     ('recolor_luma', 1.5), ('recolor_luma', 'x'), ('recolor_luma', float('nan'))])
def test_bad_values_are_rejected_whether_on_or_off(key, bad):
    for base in ({}, dict(recolor_upper=[0.2, 0.3, 0.4])):
        opt = dict(base)
        opt[key] = bad
        with pytest.raises(ValueError, match=key):
            options.recolor_settings(opt)


def test_cli_flags_set_the_keys_and_are_validated():
    ap = sample_from_parsing.cli_parser()
    ns = ap.parse_args(['-opt', 'x.yml', '--recolor-upper', '0.9,0.1,0.2', '--recolor-outer', '0,0,0', '--recolor-feather',
                        '4', '--recolor-luma', '0.5'])
    opt = sample_from_parsing.apply_cli(defaults.sample_from_parsing(), ns)
    assert opt['recolor_upper'] == [0.9, 0.1, 0.2] and opt['recolor_outer'] == [0.0, 0.0, 0.0]
    assert options.recolor_settings(opt) == ({'upper': (0.9, 0.1, 0.2), 'outer': (0.0, 0.0, 0.0)}, 4, 0.5)
    plain = sample_from_parsing.apply_cli(defaults.sample_from_parsing(), ap.parse_args(['-opt', 'x.yml']))
    assert not any(k.startswith('recolor_') for k in plain) and dict(plain) == dict(defaults.sample_from_parsing())
    with pytest.raises(ValueError, match='recolor_lower'):
        sample_from_parsing.apply_cli(defaults.sample_from_parsing(), ap.parse_args(['-opt', 'x.yml', '--recolor-lower', '2,0,0']))
    with pytest.raises(ValueError, match='recolor_feather'):
        sample_from_parsing.apply_cli(defaults.sample_from_parsing(),
                                      ap.parse_args(['-opt', 'x.yml', '--recolor-upper', '1,0,0', '--recolor-feather', '12']))
    for bad in ('1,0', 'red', '1,0,0,0'):
        with pytest.raises(SystemExit):
            ap.parse_args(['-opt', 'x.yml', '--recolor-upper', bad])


class _Stub(sample_model.SampleFromParsingModel):
    """sample_and_refine's host logic without a device: the sampler and the decoder are stand-ins"""

    def __init__(self, opt):  # (no checkpoints, no GPU)
        self.opt, self.batch_size, self.sample_steps, self.device = opt, 2, 4, 'cpu'
        self.texture_mask = torch.zeros(2, 1, 8, 8)
        self.segm = torch.ones(2, 1, 8, 8)
        self.decoded = 0

    def sample_fn(self, **kw):
        return [torch.zeros(2, 4, dtype=torch.int64)]

    def decode_indices(self, lists, want_u8=False, **kw):
        self.decoded += 1
        b = lists[0].shape[0]
        return torch.full((b, 3, 8, 8), 0.5), (torch.zeros(b, 8, 8, 3, dtype=torch.uint8) if want_u8 else None)


def test_without_the_keys_the_new_ops_are_not_called(monkeypatch, tmp_path):
    def boom(*a, **kw):
        raise AssertionError('the recolouring ran without a recolor_* option')
    monkeypatch.setattr(ops, 'region_color_stats', boom)
    monkeypatch.setattr(ops, 'recolor_region', boom)
    model = _Stub(defaults.sample_from_parsing())
    img = model.sample_and_refine()
    assert tuple(img.shape) == (1, 3, 8, 8) and model.decoded == 1
    model.sample_and_refine(str(tmp_path), ['a.png', 'b.png'])
    assert model.decoded == 2 and (tmp_path / 'a.png').exists() and (tmp_path / 'b.png').exists()
    # with a key set the same calls do enter it
    model = _Stub(defaults.with_recolor(defaults.sample_from_parsing(), upper=(1, 0, 0)))
    with pytest.raises(AssertionError, match='recolouring ran'):
        model.sample_and_refine()
    with pytest.raises(AssertionError, match='recolouring ran'):
        model.sample_and_refine(str(tmp_path), ['c.png', 'd.png'])
    assert not (tmp_path / 'c.png').exists()


def test_recolor_arguments_are_validated_before_any_kernel(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError('a kernel was reached')
    monkeypatch.setattr(ops, 'region_color_stats', boom)
    monkeypatch.setattr(ops, 'recolor_region', boom)
    model = _Stub(defaults.sample_from_parsing())
    img = torch.zeros(2, 3, 8, 8)
    for kw, word in ((dict(), 'at least one group'), (dict(upper=(1, 0)), 'colour'), (dict(upper=(2, 0, 0)), 'colour'),
                     (dict(upper=True), 'colour'), (dict(upper=torch.zeros(3, 3)), r'\[2, 3\]'),
                     (dict(upper=(1, 0, 0), feather=9), 'feather'), (dict(upper=(1, 0, 0), luma=2), 'luma'),
                     (dict(upper=(1, 0, 0), gain_max=0), 'gain_max'),
                     (dict(upper=(1, 0, 0), labels={'shirt': ([4], (0, 1, 0))}), 'disjoint'),
                     (dict(labels={'hat': [7]}), 'label ids'), (dict(labels={'hat': ([70], (0, 0, 0))}), 'label ids'),
                     (dict(upper=(1, 0, 0), like=(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8))), 'named by True'),
                     (dict(upper=True, like=torch.zeros(1, 3, 8, 8)), 'like must be'),
                     (dict(upper=True, like=(torch.zeros(3, 3, 8, 8), torch.zeros(3, 8, 8))), 'like must be')):
        with pytest.raises(ValueError, match=word):
            model.recolor(img, **kw)
    with pytest.raises(ValueError, match='img must be'):
        model.recolor(torch.zeros(2, 3, 16, 16), upper=(1, 0, 0))
    with pytest.raises(ValueError, match='img must be'):
        model.garment_colors(torch.zeros(1, 3, 8, 8))
