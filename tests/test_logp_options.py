"""Per-token log-probabilities and best-of-N: the surface without a GPU -- the YAML key `sample_best_of`,
defaults.with_best_of, the command-line flag, validation before anything is drawn, the graph keys, the C-ABI fields and
the float64 reference's own selection rule."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from text2human_amd import defaults, options

import logp_ref as ref  # noqa: E402


def test_best_of_value_validates():
    assert options.best_of_value(1) == 1 and options.best_of_value(np.int64(4)) == 4
    for bad in (0, -3, 2.0, '3', True, None):
        with pytest.raises(ValueError, match='sample_best_of.*' + repr(bad).replace('.', r'\.')):
            options.best_of_value(bad)


def test_option_key_and_with_best_of():
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    assert options.sampling_best_of(opt) == 1                                    # absent key: the existing path
    defaults.with_best_of(opt, 4)
    assert opt['sample_best_of'] == 4 and options.sampling_best_of(opt) == 4
    defaults.with_best_of(opt, 1)
    assert 'sample_best_of' not in opt and options.sampling_best_of(opt) == 1
    with pytest.raises(ValueError, match='-2'):
        defaults.with_best_of(opt, -2)
    opt['sample_best_of'] = 2.5
    with pytest.raises(ValueError, match=r'2\.5'):
        options.sampling_best_of(opt)


def test_yaml_round_trip(tmp_path):
    opt = defaults.with_best_of(defaults.sample_from_parsing(), 3)
    path = defaults.write_yaml(opt, str(tmp_path / 'o.yml'))
    back = options.dict_to_nonedict(options.parse(path, root=str(tmp_path)))
    assert options.sampling_best_of(back) == 3


def test_cli_flag_reaches_the_options():
    from text2human_amd import sample_from_parsing as sp
    args = sp.cli_parser().parse_args(['-opt', 'x.yml', '--best-of', '4', '--top-k', '48'])
    opt = sp.apply_cli(options.dict_to_nonedict({'sample_best_of': 2}), args)
    assert opt['sample_best_of'] == 4 and opt['sample_top_k'] == 48
    opt = sp.apply_cli(options.dict_to_nonedict({'sample_best_of': 2}), sp.cli_parser().parse_args(['-opt', 'x.yml']))
    assert opt['sample_best_of'] == 2                                            # the YAML's value stays
    assert sp.apply_cli(options.dict_to_nonedict({}), sp.cli_parser().parse_args(['-opt', 'x']))['sample_best_of'] is None
    with pytest.raises(ValueError, match='sample_best_of.*0'):
        sp.apply_cli(options.dict_to_nonedict({}), sp.cli_parser().parse_args(['-opt', 'x', '--best-of', '0']))
    from text2human_amd import sample_from_pose
    assert sample_from_pose.run is sp.run                                        # the pose entry point: the same flag


def test_graph_keys_without_the_flag_are_what_they_were():
    from text2human_amd import engine
    base = dict(B=8, T=512, sample_steps=256, maxr=64, temp=1.0, mask_id=18432, n_books=18, x8=True)
    plain = engine.round_graph_key(**base)
    assert plain == (8, 512, 256, 64, 1.0, 18432, 18, True, 0, 0)                # the key before the flag existed
    assert engine.round_graph_key(**base, logp=False) == plain
    assert engine.round_graph_key(**base, logp=True) == plain + ('logp', )
    assert engine.round_graph_key(**base, trunc=(64, 0), logp=True) != engine.round_graph_key(**base, logp=True)
    per = dict(B=8, T=512, sample_steps=256, maxr=64, mask_id=18432, n_books=18, x8=True)
    plain = engine.round_graph_key_per_image(**per)
    assert plain == (8, 512, 256, 64, 18432, 18, True, 'per-sample')
    assert engine.round_graph_key_per_image(**per, logp=False) == plain
    assert engine.round_graph_key_per_image(**per, logp=True) == plain + ('logp', )


def test_the_flag_is_off_by_default_on_every_surface():
    from text2human_amd import engine, ops
    from text2human_amd.models import sample_model
    for fn in (engine.sample_tokens, engine.sample_tokens_confidence, sample_model.BaseSampleModel.sample_fn,
               sample_model.BaseSampleModel.sample_fn_confidence, sample_model.BaseSampleModel.resample_fn):
        assert inspect.signature(fn).parameters['return_logp'].default is False, fn
    for fn in (ops.sample_heads, ops.confidence_commit):
        assert inspect.signature(fn).parameters['logp'].default is None, fn
    assert inspect.signature(engine.RoundGraph.__init__).parameters['logp'].default is False
    assert callable(ops.logp_summary) and callable(sample_model.BaseSampleModel.sample_best_of)


def test_the_c_structs_end_with_the_logp_pointer():
    from text2human_amd import _lib
    for cls in (_lib.SampleHeadsArgs, _lib.ConfidenceCommitArgs):
        name, typ = cls._fields_[-1]
        assert name == 'logp' and typ is ctypes.c_void_p
        assert getattr(cls, 'logp').offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(cls)
        assert cls().logp is None                                                # a zero-initialised struct: off
    assert _lib.SIGNATURES['t2h_logp_summary'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] +
                                                   [ctypes.c_void_p] * 4)


def test_best_of_validates_before_anything_is_drawn():
    from text2human_amd.models.sample_model import BaseSampleModel
    m = BaseSampleModel.__new__(BaseSampleModel)                                 # (no device: nothing may be touched)
    state = torch.get_rng_state()
    for bad in (0, 1.5, None):
        with pytest.raises(ValueError, match='sample_best_of'):
            m.sample_best_of(bad)
    m.opt = options.dict_to_nonedict({})
    with pytest.raises(ValueError, match='order'):
        m.sample_best_of(2, order='sideways')
    assert torch.equal(torch.get_rng_state(), state)


def test_reference_selection_rule():
    lp = np.full((3, 2, 4), np.nan, dtype=np.float32)
    lp[0, 0] = [-1, -1, -1, -1]
    lp[1, 0] = [-0.5, np.nan, -0.5, np.nan]                                      # the mean is per DRAWN token
    lp[2, 0] = [-0.5, -0.5, -0.5, -0.5]                                          # a tie with candidate 1: the earlier one
    lp[1, 1] = [-3, -3, -3, -3]                                                  # candidates 0 and 2 drew nothing: -inf
    choice, score = ref.best_of(lp)
    assert choice.tolist() == [1, 1] and score.tolist() == [-0.5, -3.0]
    s, c, m, _ = ref.summary(lp[1])
    assert c.tolist() == [2, 4] and s.tolist() == [-1.0, -12.0] and m.tolist() == [-0.5, -3.0]
    assert ref.best_of(np.full((2, 1, 4), np.nan, dtype=np.float32))[0].tolist() == [0]
