"""t2h_region_color_stats / t2h_recolor_region_f32 in the built library, without a GPU: the symbols are exported and
bound with the header's argument lists, their arguments are checked before any HIP call, and the host side of
ops.region_color_stats / ops.recolor_region (groups, parameters) raises what DESIGN.md 4.6l states."""
import ctypes
import os
import re

import pytest
import torch

from text2human_amd import _lib, build, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('t2h_region_color_stats', 't2h_recolor_region_f32')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_source_is_part_of_the_build():
    assert 'recolor.hip' in build.SOURCES and all(n in _lib.SIGNATURES for n in NAMES)


@pytest.mark.parametrize('name', NAMES)
def test_binding_matches_the_header(name):
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 't2h_hip.h')).read(), flags=re.S)
    m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)\s*;', src)
    assert m, name
    want = []
    for arg in m.group(1).split(','):
        arg = ' '.join(arg.split())
        if '*' in arg:
            want.append(ctypes.c_void_p)
        else:
            want.append({'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}[arg.split()[0]])
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and list(args) == want


def test_symbols_are_exported(lib):
    for name in NAMES:
        assert hasattr(lib, name), name


def test_argument_validation_without_gpu(lib):
    bad = 0x1000  # (never dereferenced: every call below is rejected on the host)
    two = (ctypes.c_uint64 * 2)(0b10010, 0b101000)
    overlap = (ctypes.c_uint64 * 2)(0b10010, 0b10000)

    def apply(img=bad, segm=bad, bits=two, G=2, src=bad, dst=bad, luma=1.0, gain_max=4.0, feather=2, out=bad + 32, B=1,
              H=512, W=256):
        return lib.t2h_recolor_region_f32(img, 1, segm, bits, G, src, dst, luma, gain_max, feather, out, None, B, H, W, None)

    for kw, word in ((dict(img=None), b'NULL'), (dict(segm=None), b'NULL'), (dict(bits=None), b'NULL'),
                     (dict(src=None), b'NULL'), (dict(dst=None), b'NULL'), (dict(out=None), b'NULL'),
                     (dict(out=bad), b'alias'), (dict(G=0), b'groups'), (dict(G=5), b'groups'),
                     (dict(bits=overlap), b'disjoint'), (dict(feather=-1), b'feather'), (dict(feather=9), b'feather'),
                     (dict(luma=-0.5), b'luma'), (dict(luma=1.5), b'luma'), (dict(luma=float('nan')), b'luma'),
                     (dict(gain_max=0.5), b'gain_max'), (dict(gain_max=17.0), b'gain_max'), (dict(B=0), b'shape'),
                     (dict(H=0), b'shape'), (dict(W=-3), b'shape')):
        assert apply(**kw) == -1, kw
        assert word in lib.t2h_last_error(), (kw, lib.t2h_last_error())

    def stats(img=bad, segm=bad, bits=two, G=2, partial=bad, out=bad, B=1, H=512, W=256):
        return lib.t2h_region_color_stats(img, 1, segm, bits, G, B, H, W, partial, out, None)

    for kw, word in ((dict(img=None), b'NULL'), (dict(segm=None), b'NULL'), (dict(bits=None), b'NULL'),
                     (dict(partial=None), b'NULL'), (dict(out=None), b'NULL'), (dict(G=0), b'groups'),
                     (dict(G=5), b'groups'), (dict(bits=overlap), b'disjoint'), (dict(B=0), b'shape'),
                     (dict(H=-1), b'shape'), (dict(W=0), b'shape')):
        assert stats(**kw) == -1, kw
        assert word in lib.t2h_last_error(), (kw, lib.t2h_last_error())


def test_group_names_and_label_lists():
    assert ops.recolor_group_bits(['upper', 'lower', 'outer']) == [0b10010, (1 << 3) | (1 << 5) | (1 << 21), 0b100]
    assert ops.recolor_group_bits([[0, 63], (7, )]) == [1 | (1 << 63), 1 << 7]
    assert ops.RECOLOR_GROUPS == {'upper': (1, 4), 'lower': (3, 5, 21), 'outer': (2, )}
    for bad in ([], ['upper'] * 5, 'upper', ['hat'], [[1], [1, 2]], ['upper', [4]], [[64]], [[-1]], [[1.5]], [[True]], [[]],
                [3], None):
        with pytest.raises(ValueError, match='recolor'):
            ops.recolor_group_bits(bad)


@pytest.mark.parametrize('kw,word', [(dict(feather=-1), 'feather'), (dict(feather=9), 'feather'), (dict(feather=2.0), 'feather'),
                                     (dict(feather=True), 'feather'), (dict(luma=-0.1), 'luma'), (dict(luma=1.1), 'luma'),
                                     (dict(luma='1'), 'luma'), (dict(luma=float('nan')), 'luma'),
                                     (dict(gain_max=0.9), 'gain_max'), (dict(gain_max=16.5), 'gain_max'),
                                     (dict(gain_max=None), 'gain_max')])
def test_parameters_are_checked_on_the_host(kw, word):
    args = dict(luma=1.0, gain_max=4.0, feather=2)
    ops._check_recolor_params(**args)
    with pytest.raises(ValueError, match=word):
        ops._check_recolor_params(**dict(args, **kw))


def test_ops_reject_bad_groups_and_parameters_before_touching_tensors():
    x, s, st = torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8), torch.zeros(1, 1, 8, dtype=torch.float64)
    with pytest.raises(ValueError, match='disjoint'):
        ops.region_color_stats(x, s, [[1, 4], [4]])
    with pytest.raises(ValueError, match='feather'):
        ops.recolor_region(x, s, ['upper'], st, st, feather=9)
    with pytest.raises(ValueError, match='unknown group'):
        ops.recolor_region(x, s, ['sleeves'], st, st)
    with pytest.raises(TypeError):            # (host tensors: there is no CPU path)
        ops.region_color_stats(x, s, ['upper'])


def test_colour_space_round_trip():
    c = torch.rand(5, 3, dtype=torch.float64)
    yuv = ops.recolor_yuv(c)
    assert torch.allclose(yuv[:, 0], 0.299 * c[:, 0] + 0.587 * c[:, 1] + 0.114 * c[:, 2])
    assert torch.allclose(ops.recolor_rgb(yuv), c, atol=1e-14)
    assert torch.allclose(ops.recolor_yuv((0.5, 0.5, 0.5)), torch.tensor([0.5, 0.0, 0.0], dtype=torch.float64), atol=1e-15)
