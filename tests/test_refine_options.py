"""Sampled bottom-index refinement: the option surface without a GPU -- the validation helper, the
YAML keys `refine_temp` / `refine_top_k` / `refine_top_p`, defaults.with_refine_sampling, the command-line flags and
the public signatures."""
import inspect

import numpy as np
import pytest
import torch

from text2human_amd import defaults, options


def test_absent_keys_leave_sampling_off():
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    assert options.refine_sampling(opt) is None and options.refine_values() is None
    assert options.refine_values(None, None, None, batch=4) is None
    assert not any(k in opt for k in options.REFINE_KEYS)


def test_any_one_key_turns_sampling_on_with_temp_one():
    assert options.refine_values(top_k=40) == (1.0, 40, None)
    assert options.refine_values(top_p=0.9) == (1.0, None, 0.9)
    assert options.refine_values(0.7) == (0.7, None, None)
    assert options.refine_values([1.0, 0.5], None, [None, 0.9], batch=2) == ([1.0, 0.5], None, [None, 0.9])
    assert options.refine_values(top_k=1024, top_p=1.0) == (1.0, 1024, 1.0)     # spelled off, still a draw at temp 1


def test_option_keys_and_with_refine_sampling():
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    defaults.with_refine_sampling(opt, temp=0.8, top_k=64, top_p=0.9)
    assert (opt['refine_temp'], opt['refine_top_k'], opt['refine_top_p']) == (0.8, 64, 0.9)
    assert options.refine_sampling(opt) == (0.8, 64, 0.9)
    defaults.with_refine_sampling(opt, top_p=0.5)
    assert options.refine_sampling(opt) == (1.0, None, 0.5) and 'refine_temp' not in opt and 'refine_top_k' not in opt
    defaults.with_refine_sampling(opt)
    assert options.refine_sampling(opt) is None
    with pytest.raises(ValueError, match='refine_top_k.*-4'):
        defaults.with_refine_sampling(opt, top_k=-4)
    opt['refine_top_p'] = 1.75
    with pytest.raises(ValueError, match=r'refine_top_p.*1\.75'):
        options.refine_sampling(opt)


def test_yaml_round_trip(tmp_path):
    opt = defaults.with_refine_sampling(defaults.sample_from_parsing(), temp=1.2, top_k=32, top_p=0.95)
    path = defaults.write_yaml(opt, str(tmp_path / 'o.yml'))
    back = options.dict_to_nonedict(options.parse(path, root=str(tmp_path)))
    assert options.refine_sampling(back) == (1.2, 32, 0.95)
    back['refine_temp'] = [1.0, 0.5]                                # the options are scalars, like sample_top_k
    with pytest.raises(ValueError, match='refine_temp.*one value'):
        options.refine_sampling(back)


def test_cli_flags_reach_the_options():
    from text2human_amd import sample_from_parsing as sp
    args = sp.cli_parser().parse_args(['-opt', 'x.yml', '--refine-temp', '0.8', '--refine-top-k', '48', '--refine-top-p', '0.9'])
    opt = sp.apply_cli(options.dict_to_nonedict({'refine_top_k': 5}), args)
    assert (opt['refine_temp'], opt['refine_top_k'], opt['refine_top_p']) == (0.8, 48, 0.9)
    assert opt['sample_top_k'] is None and opt['sample_order'] is None                       # the sampler's keys: untouched
    opt = sp.apply_cli(options.dict_to_nonedict({'refine_top_k': 5}), sp.cli_parser().parse_args(['-opt', 'x.yml']))
    assert opt['refine_top_k'] == 5 and opt['refine_temp'] is None                           # the YAML's value stays
    assert options.refine_sampling(opt) == (1.0, 5, None)
    opt = sp.apply_cli(options.dict_to_nonedict({}), sp.cli_parser().parse_args(['-opt', 'x.yml']))
    assert options.refine_sampling(opt) is None
    for flag, value, name in (('--refine-temp', '0', 'refine_temp'), ('--refine-temp', '-1.5', 'refine_temp'),
                              ('--refine-top-p', '1.5', 'refine_top_p'), ('--refine-top-p', '0', 'refine_top_p'),
                              ('--refine-top-k', '-3', 'refine_top_k')):
        with pytest.raises(ValueError, match=name):
            sp.apply_cli(options.dict_to_nonedict({}), sp.cli_parser().parse_args(['-opt', 'x', f'{flag}={value}']))
    from text2human_amd import sample_from_pose
    assert sample_from_pose.run is sp.run                                                    # the pose entry point: the same flags


BAD = [
    (dict(temp=0.0), 'refine_temp'), (dict(temp=-2.0), 'refine_temp'), (dict(temp=float('nan')), 'refine_temp'),
    (dict(temp=float('inf')), 'refine_temp'), (dict(temp='1.0'), 'refine_temp'), (dict(temp=True), 'refine_temp'),
    (dict(top_p=0.0), 'refine_top_p'), (dict(top_p=1.5), 'refine_top_p'), (dict(top_p=-0.1), 'refine_top_p'),
    (dict(top_p=1e-9), 'refine_top_p.*too small'),
    (dict(top_k=-1), 'refine_top_k'), (dict(top_k=2.5), 'refine_top_k'),
    (dict(temp=[1.0, 0.5]), 'refine_temp: one entry per image.*2 entries'),
    (dict(top_k=[5, 5, 5, 5]), 'refine_top_k: one entry per image.*4 entries'),
    (dict(top_p=np.ones((3, 1))), 'refine_top_p.*1-D'),
    (dict(temp=[1.0, 0.0, 1.0]), 'refine_temp, image 1'),
    (dict(temp=torch.tensor([1.0, 1.0, -1.0])), 'refine_temp, image 2'),
    (dict(top_k=[None, -1, 3]), 'refine_top_k, image 1'),
    (dict(top_p=[0.5, 0.5, 1.5]), 'refine_top_p, image 2'),
]


@pytest.mark.parametrize('kw,who', BAD, ids=[f'{list(k)[0]}-{i}' for i, (k, _) in enumerate(BAD)])
def test_bad_values_raise_a_value_error_that_names_the_option(kw, who):
    with pytest.raises(ValueError, match=who):
        options.refine_values(**kw, batch=3)


def test_wrong_values_in_the_yaml_end_the_run_before_the_checkpoints_are_read():
    for key, v in (('refine_temp', 0), ('refine_top_p', 2), ('refine_top_k', -7), ('refine_temp', [1.0, -1.0])):
        with pytest.raises(ValueError, match=key):
            options.refine_sampling(options.dict_to_nonedict({key: v}))


def test_the_public_calls_take_the_three_arguments():
    from text2human_amd.models.sample_model import BaseSampleModel as M
    for fn in (M.decode_indices, M.bot_index_prediction, M.edit_and_refine):
        p = inspect.signature(fn).parameters
        assert all(p[k].default is None for k in options.REFINE_KEYS), fn.__name__
    assert inspect.signature(M._bot_indices).parameters['refine'].default is None


def test_the_model_validates_before_it_draws():
    """_refine_draw raises on a bad value or a wrong length without a device (nothing has been read or drawn)"""
    from text2human_amd.models.sample_model import BaseSampleModel as M
    m = M.__new__(M)
    assert m._refine_draw(2, None, None, None) is None
    state = torch.get_rng_state()
    for kw, who in ((dict(refine_temp=0.0), 'refine_temp'), (dict(refine_top_p=[0.5, 0.5, 0.5]), 'refine_top_p'),
                    (dict(refine_top_k=[1, -1]), 'refine_top_k, image 1')):
        with pytest.raises(ValueError, match=who):
            m._refine_draw(2, **{k: kw.get(k) for k in options.REFINE_KEYS})
    assert torch.equal(torch.get_rng_state(), state)
    assert M._refine_first_image(dict(refine_temp=[1.0, 0.5], refine_top_k=40, refine_top_p=np.array([0.9, 0.8]))) == dict(
        refine_temp=[1.0], refine_top_k=40, refine_top_p=[0.9])
