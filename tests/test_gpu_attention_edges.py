"""The attention kernels at the extremes of the score distribution (-m gpu; tests/attention_cases.py): the split-plane
flash attention in both of its forms, the exact-fp32 attention and the decoder's spatial attention, against fp64.  The
bar of the transformer kernels: no worse than twice what eager fp32 softmax(q k^T / 8) v on the device loses on the same
input + 5e-6 of the value scale; of the spatial attention, its existing test's own relation to the materialised
bgemm -> softmax -> bgemm form.  Every (case, kernel, err, err_eager) is printed (profiles/attention_edge_cases.log)."""
import pytest
import torch

import attention_cases as AC
from split_ref import pack_vt_host
from text2human_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'

B, T, H = 2, 512, 2
C = 64 * H
CASES = {name: (q, k, v) for name, q, k, v in AC.cases(B, T, H, seed=200)}
SPLIT_OUT = ['spike@%d' % (T - 1), 'onehot']
_REF = {}


def references(name):
    """(fp64 reference, error of the eager fp32 sequence on the device) of a case, computed once"""
    if name not in _REF:
        q, k, v = CASES[name]
        ref = AC.reference_fp64(q, k, v, B, T, H)
        _REF[name] = ref, AC.max_err(AC.eager_fp32(q.to(DEV), k.to(DEV), v.to(DEV), B, T, H), ref)
    return _REF[name]


def run_split(form, q, k, v, out_split=False):
    qk_s = ops.split_rows(torch.cat([q, k], dim=1).to(DEV))
    vt = pack_vt_host(v.contiguous(), B, T, H).to(DEV)
    y = torch.full((B * T, C), float('nan'), device=DEV)
    lib = _lib.load()
    lib.t2h_mha_split_force_form(form)
    try:
        ops.mha_split(qk_s, 2 * C, vt, B, T, H, out=y)
        ys = ops.mha_split(qk_s, 2 * C, vt, B, T, H, out_split=ops.split_rows_empty(B * T, C, DEV)) if out_split else None
    finally:
        lib.t2h_mha_split_force_form(0)
    return y, ys


@pytest.mark.parametrize('kernel', ['split-key-halves', 'split-all-keys', 'exact-fp32'])
@pytest.mark.parametrize('name', list(CASES))
def test_attention_at_score_extremes(name, kernel):
    q, k, v = CASES[name]
    ref, err_eager = references(name)
    if kernel == 'exact-fp32':
        y = ops.mha_noncausal(torch.cat([q, k, v], dim=1).to(DEV), B, T, H)
    else:
        ops.split_overflow(reset=True)
        y, ys = run_split(2 if kernel == 'split-key-halves' else 1, q, k, v, out_split=name in SPLIT_OUT)
        if ys is not None:   # the split-row output is the split of the fp32 output, bit for bit
            assert torch.equal(ys, ops.split_rows(y)) and ops.split_overflow_bits(reset=True) == 0
    err = AC.max_err(y, ref)
    print(f'{name:12s} {kernel:16s} err {err:.3e} eager {err_eager:.3e} allowed {AC.allowed(err_eager, v):.3e}')
    assert torch.isfinite(y).all(), (name, kernel)
    assert AC.bar(err, err_eager, v), (name, kernel, err, err_eager)
    if name in AC.UNIFORM:
        assert AC.max_err(y, AC.v_mean(v, B, T, H)) <= 1e-6 * float(v.abs().max()), (name, kernel)


@pytest.mark.parametrize('n_img,N,C', [(2, 512, 256), (1, 96, 256)])
def test_spatial_attention_at_score_extremes(n_img, N, C):
    """t2h_spatial_attention_f32 skips the rescale of its accumulators when no lane's alpha differs from 1: dominant keys
    at N/2-1, N/2, N-1 (position 5 is in test_spatial_attention_matches_fp64_and_the_materialised_form), rising and
    falling scores, one-hot and uniform softmax, each next to the materialised form"""
    scale = float(int(C) ** (-0.5))
    for name, qkv in AC.spatial_cases(n_img, N, C, seed=300 + N):
        q, k, v = [t.reshape(n_img, N, C).double() for t in qkv.split(C, dim=1)]
        ref = (torch.softmax(q @ k.transpose(1, 2) * scale, -1) @ v).reshape(n_img * N, C)
        d = qkv.to(DEV)
        got = ops.spatial_attention(d, n_img, N, C)
        q3 = d.view(n_img, N, 3 * C)
        s = torch.empty((n_img, N, N), device=DEV)
        ops.bgemm(q3[:, :, :C], q3[:, :, C:2 * C], s, alpha=scale)
        ops.softmax_rows_(s)
        mat = torch.empty((n_img, N, C), device=DEV)
        ops.bgemm(s, q3[:, :, 2 * C:], mat, b_trans=True)
        e_new, e_old = AC.max_err(got, ref), AC.max_err(mat.view(-1, C), ref)
        vscale = max(1.0, float(v.abs().max()))
        print(f'{name:12s} spatial N={N:<5d} err {e_new:.3e} materialised {e_old:.3e} allowed {2e-5 * vscale + 3 * e_old:.3e}')
        assert torch.isfinite(got).all(), name
        assert e_new < 2e-5 * vscale + 3 * e_old, (name, e_new, e_old)
        if name == 'uniform_q0':
            mean = v.mean(dim=1, keepdim=True).expand(n_img, N, C).reshape(n_img * N, C)
            assert AC.max_err(got, mean) <= 1e-6 * float(v.abs().max()), name
