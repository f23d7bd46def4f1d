"""The transformer's attention kernels on the CPU (csrc/attention.hip through tests/emu) at the extremes of the score
distribution (tests/attention_cases.py): the dominant key in the first tile, at the end of key half 0, at the start of
key half 1, in the last tile; maxima that move in every tile, in none, in a different tile per lane; uniform and one-hot
softmax; scores whose rescale factor underflows to 0.  B, T, H = 1, 256, 1 is the smallest shape with two key halves of
two tiles each.  The bar: no worse than twice the reference's own fp32 operator sequence (torch on the CPU) on the same
input + 5e-6 of the value scale, and finite."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import build_emu  # noqa: E402

import attention_cases as AC  # noqa: E402
from split_ref import pack_vt_host  # noqa: E402
from text2human_amd import ops  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')

B, T, H = 1, 256, 1
C = 64 * H
CASES = {name: (q, k, v) for name, q, k, v in AC.cases(B, T, H, seed=100)}
LATE = ['spike@%d' % (T - 1), 'rise', 'fall']      # also with the LDS-DMA requests landing only at the kernel's waits
KERNELS = ['split-key-halves', 'split-all-keys', 'exact-fp32']

_REF = {}


def references(name):
    """(fp64 reference, error of the eager fp32 sequence) of a case, computed once"""
    if name not in _REF:
        q, k, v = CASES[name]
        ref = AC.reference_fp64(q, k, v, B, T, H)
        _REF[name] = ref, AC.max_err(AC.eager_fp32(q, k, v, B, T, H), ref)
    return _REF[name]


@pytest.fixture(scope='module')
def lib():
    so = build_emu.load('attention.hip')
    yield so
    so.emu_set_deferred(0)


def launch(lib, kernel, q, k, v):
    y = torch.full((B * T, C), float('nan'))
    if kernel == 'exact-fp32':
        qkv = torch.cat([q, k, v], dim=1).contiguous()
        rc = lib.t2h_mha_noncausal_f32(qkv.data_ptr(), y.data_ptr(), B, T, H, None)
    else:
        qk = ops.pack_split_rows_host(torch.cat([q, k], dim=1))
        vt = pack_vt_host(v.contiguous(), B, T, H)
        old = lib.t2h_mha_split_force_form(2 if kernel == 'split-key-halves' else 1)
        try:
            rc = lib.t2h_mha_split_f32(qk.data_ptr(), 2 * C, vt.data_ptr(), y.data_ptr(), None, B, T, H, None, None)
        finally:
            lib.t2h_mha_split_force_form(old)
    assert rc == 0, lib.emu_last_error()
    return y


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('name,deferred', [(n, 0) for n in CASES] + [(n, 1) for n in LATE],
                         ids=list(CASES) + [n + '-requests-land-at-the-wait' for n in LATE])
def test_emulated_attention_at_score_extremes(lib, name, deferred, kernel):
    q, k, v = CASES[name]
    ref, err_eager = references(name)
    lib.emu_set_deferred(deferred)
    try:
        y = launch(lib, kernel, q, k, v)
    finally:
        lib.emu_set_deferred(0)
    err = AC.max_err(y, ref)
    print(f'{name:12s} {kernel:16s} err {err:.3e} eager {err_eager:.3e} allowed {AC.allowed(err_eager, v):.3e}')
    assert torch.isfinite(y).all(), (name, kernel)
    assert AC.bar(err, err_eager, v), (name, kernel, err, err_eager)
    if name in AC.UNIFORM:
        assert AC.max_err(y, AC.v_mean(v, B, T, H)) <= 1e-6 * float(v.abs().max()), (name, kernel)
