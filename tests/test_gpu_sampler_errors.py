"""What the two sampling loops refuse (-m gpu): engine.sample_tokens and engine.sample_tokens_confidence raise on a bad
argument before anything is drawn -- the device generator stays where it was -- and before the transformer is evaluated."""
import pytest
import torch

from text2human_amd import engine, synthetic, weights
from text2human_amd._lib import T2HError

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MASK_ID, N_BOOKS, N_CLASS, B, T = 18432, 18, 1024, 2, 512
BAD_ROW = (1, 77)   # (sample, token row) of the kept row without a source token


@pytest.fixture(scope='module')
def net():
    sd = synthetic.fill(synthetic.transformer_schema(MASK_ID, N_CLASS, N_BOOKS, 512, 1, T, N_BOOKS), seed=12)
    P = weights.Params(DEV)
    net = engine.SamplerNet(P, weights.pack_transformer(P, sd, 'tf'), 8, 'tf', split=True, x8=False)

    def hidden(*a, **kw):
        raise AssertionError('the transformer was evaluated')
    net.hidden = hidden
    return net


def _inputs():
    g = torch.Generator().manual_seed(5)
    segm = torch.randint(0, 1024, (B, T), generator=g).to(DEV)
    tex = torch.randint(0, N_BOOKS, (B, T), generator=g).to(DEV)
    src = torch.randint(0, N_CLASS, (N_BOOKS, B * T), generator=g).to(DEV)
    keep = torch.ones(B * T, dtype=torch.uint8, device=DEV)
    return segm, tex, src, keep


def _bad_texture_id(segm, tex, src, keep):
    tex = tex.clone()
    tex[1, 3] = N_BOOKS
    return (segm, tex), {}, T2HError, 'texture ids'


def _bad_init_shape(segm, tex, src, keep):
    return (segm, tex), dict(init=(src, keep[:-1].contiguous())), ValueError, 'init: source lists'


def _bad_top_p(segm, tex, src, keep):
    return (segm, tex), dict(top_p=0), ValueError, 'top_p'


def _kept_row_without_source(segm, tex, src, keep):
    b, j = BAD_ROW
    src = src.clone()
    src[tex[b, j], b * T + j] = -1
    return (segm, tex), dict(init=(src, keep)), T2HError, f'token row {j} of sample {b}'


@pytest.mark.parametrize('case', [_bad_texture_id, _bad_init_shape, _bad_top_p, _kept_row_without_source])
@pytest.mark.parametrize('entry', ['sample_tokens', 'sample_tokens_confidence'])
def test_bad_argument_raises_before_the_generator_moves(net, entry, case):
    (segm, tex), kw, exc, match = case(*_inputs())
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    gen.manual_seed(11)
    torch.rand(3, device=DEV)                              # (an offset other than 0)
    off = gen.get_offset()
    with pytest.raises(exc, match=match):
        if entry == 'sample_tokens':
            engine.sample_tokens(net, segm, tex, 6, MASK_ID, **kw)
        else:
            engine.sample_tokens_confidence(net, segm, tex, MASK_ID, rounds=4, **kw)
    assert gen.get_offset() == off
