"""Sampled bottom-index refinement on the CPU: t2h_routed_head_sample of csrc/sampler.hip, and
t2h_routed_head_argmax of csrc/vq.hip beside it, from their SOURCE through tests/emu.  The property code is
tests/refine_ref.py (numbered as there); the hardware twin is tests/test_gpu_refine_sample.py.  The emulator runs every
thread of a workgroup as an OS thread, so the rows are 37 where the hardware file has 111, and the largest class
count (1024, four classes per thread) appears once per property."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))
sys.path.insert(0, HERE)
import build_emu  # noqa: E402
import decode_bands as D  # noqa: E402
import per_image_ref  # noqa: E402
import refine_ref as RR  # noqa: E402

needs_emu = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')


@functools.lru_cache(maxsize=None)
def _load(kernel_file):
    return build_emu.load(kernel_file)


ENV = D.Env('cpu', _load, lambda: None, lambda lib: lib.emu_last_error())
N = 37


def table_of(sets):
    return torch.from_numpy(per_image_ref.table(sets))


@needs_emu
def test_the_entry_point_has_the_signature_the_loader_declares():
    from text2human_amd import _lib
    so = _load('sampler.hip')
    assert so.t2h_routed_head_sample.argtypes == _lib.SIGNATURES['t2h_routed_head_sample'][1]


@needs_emu
@pytest.mark.parametrize('n_class', [37, 1024])
def test_emulated_equals_the_argmax_kernel_when_the_noise_says_nothing(n_class):
    RR.equals_argmax_when_the_noise_says_nothing(ENV, N, n_class)


@pytest.mark.parametrize('n,n_class', [(37, 37), (37, 1024), (111, 37), (111, 1024)])
def test_the_draw_seed_excuses_no_row(n, n_class):
    """the seed of property 2, on torch alone: no row of the fp64 race is a near-tie, and the fp32 restatement draws
    the fp64 one's tokens"""
    pb = RR.problem(n, n_class)
    for temp in (1.0, 0.7):
        want, near = RR.race(RR.raw64(pb) / temp, pb['expo'])
        got, _ = RR.race(RR.raw32(pb) / temp, pb['expo'])
        assert int(near.sum()) == 0 and torch.equal(got, want)


@needs_emu
@pytest.mark.parametrize('n_class', [37, 1024])
def test_emulated_draw_is_the_fp64_race(n_class):
    RR.the_draw(ENV, N, n_class)


@needs_emu
@pytest.mark.parametrize('n_class,cases,scopes', [(37, [(2, 0.5), (5, None), (None, 0.9)], (1, )), (1024, [(64, 0.9)], (0, 1))])
def test_emulated_truncation(n_class, cases, scopes):
    """(the workgroup form of t2h_truncation_threshold is 1024 OS threads per row here: once)"""
    RR.truncation(ENV, N, n_class, cases, scopes=scopes)


@needs_emu
@pytest.mark.parametrize('n_class,rules', [(37, (dict(top_k=5, top_p_q=RR.p_q_of(0.9)), )), (1024, (dict(), ))])
def test_emulated_in_kernel_noise_is_the_philox_tensor(n_class, rules):
    RR.in_kernel_noise(ENV, N, n_class, rules=rules)


@needs_emu
def test_emulated_per_sample_table():
    """three samples of 13 rows here (37 on the hardware)"""
    RR.per_sample_table(ENV, 13, 37, table_of)


def test_the_frequency_seed_passes_on_torchs_own_race():
    """the seed of property 6 on the CPU generator: torch's own exponential_ race stays inside the bound"""
    pb = RR.problem(RR.FREQ_ROWS, 37, seed=RR.FREQ_SEED, ties=False, repeat=True)
    e = torch.empty(RR.FREQ_ROWS, 37).exponential_(generator=torch.Generator().manual_seed(RR.FREQ_SEED))
    for temp in (1.0, 2.0):
        l = RR.raw64(pb) / temp
        tok, _ = RR.race(l, e)
        RR.binomial_bound_holds(tok, torch.softmax(l[0], 0), f'temp {temp}')


@needs_emu
def test_emulated_philox_race_samples_the_softmax():
    """property 6 on the Philox tensor the kernel computes (t2h_philox_exponential_f32 through the emulator, raced by
    the fp64 restatement: the 4096-workgroup launch itself stays with the hardware file), and the kernel on its first
    37 rows against that race"""
    pb = RR.problem(RR.FREQ_ROWS, 37, seed=RR.FREQ_SEED, ties=False, repeat=True)
    ph = (RR.FREQ_SEED, 0, RR.GRID_THREADS)
    e = RR.philox_expo(ENV, *ph, RR.FREQ_ROWS, 37)
    for temp in (1.0, 2.0):
        l = RR.raw64(pb) / temp
        tok, near = RR.race(l, e)
        RR.binomial_bound_holds(tok, torch.softmax(l[0], 0), f'temp {temp}')
        got = RR.Launch(ENV, RR.rows_of(pb, slice(0, N)), temp=temp, expo=None, philox=ph).run()
        RR.assert_tokens(got.tok, tok[:N], near[:N], 'first rows')


@needs_emu
def test_emulated_rejected_arguments_write_nothing():
    RR.rejected_arguments(ENV, table_of)
