"""The split-row producers at the edges of the formats' value range (-m gpu; tests/split_edges.py, the same inputs as
tests/test_split_edges_emulated.py): on hardware the conversions are instructions (v_cvt_f16_f32, v_cvt_pk_fp8_f32) the
emulator only restates -- every rounding tie, the exact thresholds of the overflow word; the split GEMM on operands
whose fp16 hi plane is subnormal (does the matrix pipe keep fp16 subnormals?); a near-zero weight matrix through the x8
chain, and a sampler network with a near-zero projection matrix through the x8 calibration."""
import pytest
import torch
import torch.nn.functional as F

import split_edges as E
from text2human_amd import _lib, engine, ops, synthetic, weights

pytestmark = pytest.mark.gpu
DEV = 'cuda'


class Device:
    @staticmethod
    def _bits(out):
        return out.cpu(), ops.split_overflow_bits(reset=True)

    def split_rows(self, x):
        ops.split_overflow(reset=True)
        return self._bits(ops.split_rows(x.to(DEV)))

    def split_rows_x8(self, x, s):
        ops.split_overflow(reset=True)
        return self._bits(ops.split_rows_x8(x.to(DEV), s))

    def layernorm_split(self, x, g, b):
        ops.split_overflow(reset=True)
        return self._bits(ops.layernorm_split(x.to(DEV), g.to(DEV), b.to(DEV), ops.split_rows_empty(x.shape[0], x.shape[1], DEV)))

    def layernorm_x8(self, x, g, b, s):
        ops.split_overflow(reset=True)
        return self._bits(ops.layernorm_x8(x.to(DEV), g.to(DEV), b.to(DEV), ops.split_rows_empty(x.shape[0], x.shape[1], DEV), s))

    def gemm(self, A, B, M, N, K, x8=None, cfg=-1, out_split=None):
        lib = _lib.load()
        out = torch.full((M, N), float('nan'), device=DEV)
        rows = ops.split_rows_empty(M, N, DEV) if out_split is not None else None
        ops.split_overflow(reset=True)
        lib.t2h_gemm_split_force_config(cfg)
        try:
            ops.gemm_split(A.to(DEV), B.to(DEV), M, N, K, out=out, out_split=rows, x8=x8,
                           out_x8_scale=None if out_split in (None, 'fp16') else out_split)
        finally:
            lib.t2h_gemm_split_force_config(-1)
        bits = ops.split_overflow_bits(reset=True)
        return out.cpu(), rows.cpu() if rows is not None else None, bits


@pytest.fixture(scope='module')
def be():
    return Device()


def test_fp16_plane_rounding_ladder(be):
    E.ladder_fp16_planes(be)


def test_x8_rounding_ladder(be):
    E.ladder_x8_planes(be)


def test_overflow_thresholds_of_the_producers(be):
    E.thresholds_producers(be)


def test_overflow_thresholds_of_layernorm(be):
    E.thresholds_layernorm(be)


@pytest.mark.parametrize('M', [128, 70])
def test_overflow_thresholds_of_the_gemm_epilogue(be, M):
    E.thresholds_gemm_epilogue(be, M)


@pytest.mark.parametrize('both', [False, True], ids=['w-2e-5', 'a-and-w-2e-5'])
@pytest.mark.parametrize('x8', [False, True], ids=['fp16-planes', 'x8'])
@pytest.mark.parametrize('cfg,M,N,K', E.SUBNORMAL_SHAPES)
def test_gemm_on_subnormal_hi_planes(be, cfg, M, N, K, x8, both):
    E.gemm_on_subnormal_planes(be, cfg, M, N, K, x8, both)


def test_near_zero_weight_matrix_through_the_x8_chain(be):
    E.near_zero_weight_chain(be)


def test_sampler_net_with_a_near_zero_projection_matrix_calibrates_and_matches_the_oracle():
    """one layer's attention projection scaled by 1e-7 (max |w| ~ 1e-8: its fp16 plane is all zero, the value lives in the
    residual plane): the scale of that matrix is the cap, 2^22, the packing raises no flag, and the hidden state is
    finite and within test_gpu_x8's bar of the oracle"""
    from oracle import torch_ref as R
    sd = synthetic.fill(synthetic.transformer_schema(18432, 1024, 18, 512, 6, 512, 18), seed=12)
    key = [k for k in sd if k.endswith('.attn.proj.weight')][2]
    sd[key] = sd[key] * 1e-7
    P = weights.Params(DEV)
    desc = weights.pack_transformer(P, sd, 'tf')
    gen = torch.Generator().manual_seed(14)
    idx = torch.randint(0, 18433, (3, 512), generator=gen)
    seg = torch.randint(0, 1024, (3, 512), generator=gen)
    tex = torch.randint(0, 18, (3, 512), generator=gen)
    n8 = engine.SamplerNet(P, desc, 8, 'tf', split=True, x8=True)
    ops.split_overflow(reset=True)
    a = n8.hidden(idx.to(DEV), seg.to(DEV), tex.to(DEV)).clone().cpu()
    assert n8._x8 is not None and ops.split_overflow_bits(reset=True) == 0
    scales = sorted(n8._x8['w'].values())
    assert scales[-1] == ops.X8_SCALE_MAX and scales[-2] < ops.X8_SCALE_MAX
    assert all(ops.X8_SCALE_MIN <= s <= ops.X8_SCALE_MAX for s in list(n8._x8['w'].values()) + list(n8._x8['a'].values()))
    with torch.no_grad():
        ref = R.transformer_hidden(idx, seg, tex, sd)
    ln = lambda t: F.layer_norm(t.view(3, 512, 512), (512, ), sd['ln_f.weight'], sd['ln_f.bias'], 1e-5)  # noqa: E731
    assert torch.isfinite(a).all()
    e8 = (ln(a) - ref).abs().max().item()
    print(f'near-zero proj: hidden state max abs err {e8:.3e}')
    assert e8 < 1e-4, e8
