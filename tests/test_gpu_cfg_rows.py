"""t2h_gemm_split_args.cfg_rows on the GPU (-m gpu): the dispatcher picks the tile configuration of a problem
of cfg_rows rows, and a tile configuration fixes the order in which an output element's products are summed -- so a row's
bits do not depend on how many rows the call has.  Per-image seeds rest on exactly this: the layers of a batch of B
images run with cfg_rows = T, and the last layer's tail runs with a cfg_rows that selects the few-rows kernel (M <= 64)
on up to all rows of the batch."""
import pytest
import torch

from text2human_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _problem(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    return ops.split_rows(a.to(DEV)), ops.pack_split_rows_host(w).to(DEV), b.to(DEV), r.to(DEV)


def _run(a_s, w_s, b, r, lo, hi, N, K, **kw):
    out = torch.full((hi - lo, N), float('nan'), device=DEV)
    ops.gemm_split(a_s[lo:hi], w_s, hi - lo, N, K, out=out, bias=b, residual=r[lo:hi].contiguous(), **kw)
    return out


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize('N,K', [(1536, 512), (2048, 512), (512, 2048)])   # q|k|v, fc1, fc2 of the sampler
def test_rows_of_three_images_have_the_bits_of_one_image_alone(N, K):
    T, B = 512, 3
    a_s, w_s, b, r = _problem(B * T, N, K, seed=N + K)
    whole = _run(a_s, w_s, b, r, 0, B * T, N, K, cfg_rows=T)
    for i in range(B):
        alone = _run(a_s, w_s, b, r, i * T, (i + 1) * T, N, K)               # what the dispatcher gives M = T by itself
        assert torch.equal(_bits(whole[i * T:(i + 1) * T]), _bits(alone)), i
    auto = _run(a_s, w_s, b, r, 0, B * T, N, K)
    assert torch.allclose(auto, whole, rtol=1e-4, atol=1e-4)
    if N == 1536:   # (M = 1536 leaves the in-block K split M = 512 gets: another summation order, other last bits)
        assert not torch.equal(_bits(auto), _bits(whole))


@pytest.mark.parametrize('M', [65, 200, 256, 1536])   # above the few-rows kernel's own limit; odd; the tail's buffers; a batch
@pytest.mark.parametrize('N,K', [(512, 512), (2048, 512), (512, 2048)])     # proj, fc1, fc2: the last layer's tail
def test_few_rows_kernel_on_any_row_count_gives_the_bits_of_small_calls(M, N, K):
    a_s, w_s, b, r = _problem(M, N, K, seed=M + N + K)
    whole = _run(a_s, w_s, b, r, 0, M, N, K, cfg_rows=16)
    assert bool(torch.isfinite(whole).all())
    for lo in range(0, M, 48):   # calls of at most 48 rows: the few-rows kernel by the dispatcher's own choice
        hi = min(M, lo + 48)
        small = _run(a_s, w_s, b, r, lo, hi, N, K)
        assert torch.equal(_bits(whole[lo:hi]), _bits(small)), (lo, hi)
    one = _run(a_s, w_s, b, r, M - 1, M, N, K)                               # a row alone
    assert torch.equal(_bits(whole[M - 1:]), _bits(one))
