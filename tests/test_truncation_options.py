"""Truncated sampling (top-k / top-p): the option surface without a GPU -- the one validation helper, the YAML keys
`sample_top_k` / `sample_top_p`, defaults.with_truncation, the command-line flags, the graph key."""
import pytest

from text2human_amd import defaults, options


def test_settings_helper_maps_off_and_validates():
    ts = options.truncation_settings
    assert ts() == (0, 0) and ts(None, None, 1024) == (0, 0) and ts(0, 1.0) == (0, 0)
    assert ts(1024, None, 1024) == (0, 0) and ts(5000, 1, 1024) == (0, 0)       # >= n_class / p = 1: off
    assert ts(64, 0.9, 1024) == (64, 943718) and ts(1, 0.5) == (1, 1 << 19)
    assert ts(None, 1.0 - 2.0**-22) == (0, 0)                                    # rounds to 2^20: off
    for bad in (-1, 2.5, '8', True):
        with pytest.raises(ValueError, match='top_k.*' + repr(bad).replace('.', r'\.')):
            ts(bad, None)
    for bad in (0.0, -0.25, 1.5, float('nan'), '0.9', False):
        with pytest.raises(ValueError, match='top_p.*' + repr(bad).replace('.', r'\.')):
            ts(None, bad)
    with pytest.raises(ValueError, match='too small.*1e-08'):
        ts(None, 1e-8)


def test_ops_uses_the_same_helper():
    from text2human_amd import ops
    assert ops.truncation_settings is options.truncation_settings and ops.TOP_P_ONE == 1 << 20


def test_option_keys_and_with_truncation():
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    assert options.sampling_truncation(opt) == (None, None)                      # absent keys: the reference's draw
    defaults.with_truncation(opt, top_k=64, top_p=0.9)
    assert opt['sample_top_k'] == 64 and opt['sample_top_p'] == 0.9
    assert options.sampling_truncation(opt) == (64, 0.9)
    defaults.with_truncation(opt, top_k=None, top_p=0.5)
    assert options.sampling_truncation(opt) == (None, 0.5) and 'sample_top_k' not in opt
    with pytest.raises(ValueError, match='-4'):
        defaults.with_truncation(opt, top_k=-4)
    opt['sample_top_p'] = 1.75
    with pytest.raises(ValueError, match=r'1\.75'):
        options.sampling_truncation(opt)


def test_yaml_round_trip(tmp_path):
    opt = defaults.with_truncation(defaults.sample_from_parsing(), top_k=32, top_p=0.95)
    path = defaults.write_yaml(opt, str(tmp_path / 'o.yml'))
    back = options.dict_to_nonedict(options.parse(path, root=str(tmp_path)))
    assert options.sampling_truncation(back) == (32, 0.95)


def test_cli_flags_reach_the_options():
    from text2human_amd import sample_from_parsing as sp
    args = sp.cli_parser().parse_args(['-opt', 'x.yml', '--top-k', '48', '--top-p', '0.8', '--order', 'confidence'])
    opt = sp.apply_cli(options.dict_to_nonedict({'sample_top_k': 5}), args)
    assert opt['sample_top_k'] == 48 and opt['sample_top_p'] == 0.8 and opt['sample_order'] == 'confidence'
    args = sp.cli_parser().parse_args(['-opt', 'x.yml'])
    opt = sp.apply_cli(options.dict_to_nonedict({'sample_top_k': 5}), args)
    assert opt['sample_top_k'] == 5 and opt['sample_top_p'] is None              # the YAML's value stays
    with pytest.raises(ValueError, match=r'1\.5'):
        sp.apply_cli(options.dict_to_nonedict({}), sp.cli_parser().parse_args(['-opt', 'x', '--top-p', '1.5']))
    from text2human_amd import sample_from_pose
    assert sample_from_pose.run is sp.run                                        # the pose entry point: the same flags


def test_graph_key_differs_between_settings():
    from text2human_amd import engine, ops
    base = dict(B=8, T=512, sample_steps=256, maxr=64, temp=1.0, mask_id=18432, n_books=18, x8=True)
    keys = {engine.round_graph_key(**base, trunc=ops.truncation_settings(k, p, 1024))
            for k, p in ((None, None), (64, None), (32, None), (None, 0.9), (None, 0.5), (64, 0.9))}
    assert len(keys) == 6
    assert engine.round_graph_key(**base) == engine.round_graph_key(**base, trunc=ops.truncation_settings(1024, 1.0, 1024))
    assert engine._trunc_kw((64, 943718)) == dict(top_k=64, top_p=943718 / (1 << 20))
    assert ops.truncation_settings(**engine._trunc_kw((64, 943718))) == (64, 943718)
