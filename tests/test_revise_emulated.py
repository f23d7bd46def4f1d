"""Self-correction's small kernels on the CPU: t2h_fold_keep, t2h_fold_gather, t2h_select_lowest and
t2h_accept_merge of csrc/sampler.hip through tests/emu, byte for byte against tests/revise_ref.py.

What is pinned here: the fold lattice (every non-kept row hidden by exactly one fold, a caller-kept row by none, for
K >= 4 no row sharing a fold with one of its eight neighbours), the order t2h_select_lowest selects in (value, then row
index; NaN never, -inf first, +0.0 and -0.0 tie) with every relation of count to the number of eligible rows, the
accept rule, and that none of the launches writes outside its outputs (sentinels around every buffer)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))
sys.path.insert(0, HERE)
import build_emu  # noqa: E402
import revise_ref as ref  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')

PAD = 64  # sentinel elements on either side of every output


@pytest.fixture(scope='module')
def lib():
    from text2human_amd import _lib
    so = build_emu.load('sampler.hip')
    for name in ('t2h_fold_keep', 't2h_fold_gather', 't2h_select_lowest', 't2h_accept_merge'):
        assert getattr(so, name).argtypes == _lib.SIGNATURES[name][1]
    return so


def _padded(n, dtype, fill):
    """(whole buffer, the n elements in its middle) -- the rest are sentinels"""
    whole = torch.full((n + 2 * PAD, ), fill, dtype=dtype)
    return whole, whole[PAD:PAD + n]


def _untouched(whole, fill):
    return bool((whole[:PAD] == fill).all()) and bool((whole[-PAD:] == fill).all())


def _caller_keep(B, T, seed):
    rs = np.random.RandomState(seed)
    keep = (rs.random_sample((B, T)) < 0.3).astype(np.uint8) * rs.randint(1, 256, size=(B, T)).astype(np.uint8)
    return keep  # (any nonzero value keeps)


@pytest.mark.parametrize('K', ref.FOLDS)
@pytest.mark.parametrize('th,tw,B', [(32, 16, 1), (5, 3, 2)])
@pytest.mark.parametrize('with_keep', [False, True])
def test_fold_keep(lib, K, th, tw, B, with_keep):
    T = th * tw
    keep = _caller_keep(B, T, 7 + K) if with_keep else None
    whole, out = _padded(K * B * T, torch.uint8, 0xAB)
    kt = torch.from_numpy(keep.copy()) if with_keep else None
    rc = lib.t2h_fold_keep(kt.data_ptr() if with_keep else None, K, B, th, tw, out.data_ptr(), None)
    assert rc == 0, lib.emu_last_error()
    got = out.numpy().reshape(K, B, T)
    assert got.tobytes() == ref.fold_keep(K, B, th, tw, keep).tobytes()
    assert _untouched(whole, 0xAB)
    # the properties themselves, on the kernel's output
    hidden = (got == 0).sum(0)                                                  # [B, T]: the folds that hide the row
    kept = np.zeros((B, T), bool) if keep is None else keep != 0
    assert (hidden[~kept] == 1).all() and (hidden[kept] == 0).all()
    assert set(np.unique(got)) <= {0, 1}
    if not with_keep:
        fold = (got[:, 0] == 0).argmax(0)                                       # the fold of every row
        assert sorted(set(fold.tolist())) == sorted(set(range(K)) & set(ref.fold_map(th, tw, K).tolist()))
        if K >= 4:
            for i in range(T):
                assert all(fold[j] != fold[i] for j in ref.neighbours(i, th, tw)), i


def test_fold_keep_rejects_other_fold_counts(lib):
    out = torch.zeros(16 * 512, dtype=torch.uint8)
    for K in (0, 1, 3, 5, 6, 32, -4):
        assert lib.t2h_fold_keep(None, K, 1, 32, 16, out.data_ptr(), None) != 0
    assert not bool(out.any())


@pytest.mark.parametrize('K', ref.FOLDS)
def test_fold_gather(lib, K):
    th, tw, B = 5, 3, 2
    n = B * th * tw
    rs = np.random.RandomState(K)
    logp_k = torch.from_numpy(rs.standard_normal((K, n)).astype(np.float32))
    rank_k = torch.from_numpy(rs.randint(-1, 1024, size=(K, n)).astype(np.int32))
    fold = np.tile(ref.fold_map(th, tw, K), B)
    for with_rank in (True, False):
        wl, lp = _padded(n, torch.float32, 777.0)
        wr, rk = _padded(n, torch.int32, -99)
        rc = lib.t2h_fold_gather(logp_k.data_ptr(), rank_k.data_ptr() if with_rank else None, K, B, th, tw, lp.data_ptr(),
                                 rk.data_ptr() if with_rank else None, None)
        assert rc == 0, lib.emu_last_error()
        assert lp.numpy().tobytes() == logp_k.numpy()[fold, np.arange(n)].tobytes()
        if with_rank:
            assert rk.numpy().tobytes() == rank_k.numpy()[fold, np.arange(n)].tobytes()
        else:
            assert bool((rk == -99).all())
        assert _untouched(wl, 777.0) and _untouched(wr, -99)


def _select_problem(T, seed):
    """score float32 [3, T] and the counts to try.  Image 0: runs of bit-equal values, NaN rows, -inf rows, both zeros;
    image 1: distinct values, no NaN; image 2: all NaN."""
    rs = np.random.RandomState(seed)
    s = np.empty((3, T), dtype=np.float32)
    s[0] = rs.choice(np.array([-3.5, -1.25, -0.5, -7.0], dtype=np.float32), size=T)   # long runs of equal values
    where = rs.permutation(T)
    s[0, where[:T // 10]] = np.nan
    s[0, where[T // 10:T // 10 + 5]] = -np.inf
    s[0, where[T // 10 + 5:T // 10 + 11]] = 0.0
    s[0, where[T // 10 + 11:T // 10 + 17]] = -0.0
    s[0, where[T // 10 + 17]] = np.float32(1e-30)                                # (above both zeros)
    s[1] = -rs.random_sample(T).astype(np.float32) * 9
    s[2] = np.nan
    return s


@pytest.mark.parametrize('T', [512, 100])
def test_select_lowest(lib, T):
    s = _select_problem(T, T)
    elig = [int((~np.isnan(s[b])).sum()) for b in range(3)]
    assert elig[2] == 0 and 0 < elig[0] < T and elig[1] == T
    n_inf, n_negzero = int(np.isinf(s[0]).sum()), int((np.signbit(s[0]) & (s[0] == 0)).sum())
    assert n_inf == 5 and n_negzero == 6
    # the zeros region of image 0 starts after the -inf rows and the negative values: a count that ends inside it
    below_zero = int((s[0] < 0).sum())
    counts = [(0, 0, 0), (1, 1, 1), (elig[0], elig[1], 5), (elig[0] + 7, T + 100, 1), (3, T // 4, 0),
              (below_zero + 4, 17, T), (n_inf + 2, T - 1, 2), (-3, 2, -1)]
    score = torch.from_numpy(s.copy())
    for cnt in counts:
        wk, keep_out = _padded(3 * T, torch.uint8, 0xCD)
        wn, n_sel = _padded(3, torch.int32, -55)
        c = torch.tensor(cnt, dtype=torch.int32)
        rc = lib.t2h_select_lowest(score.data_ptr(), c.data_ptr(), 3, T, keep_out.data_ptr(), n_sel.data_ptr(), None)
        assert rc == 0, lib.emu_last_error()
        want_keep, want_n = ref.select_lowest(s, cnt)
        got = keep_out.numpy().reshape(3, T)
        assert got.tobytes() == want_keep.tobytes(), cnt
        assert n_sel.numpy().tobytes() == want_n.tobytes(), cnt
        assert _untouched(wk, 0xCD) and _untouched(wn, -55)
        assert score.numpy().tobytes() == s.tobytes() and c.tolist() == list(cnt)   # the inputs are only read
        # said directly: the count, NaN rows never, the all-NaN image nothing
        assert [int((got[b] == 0).sum()) for b in range(3)] == [min(max(x, 0), e) for x, e in zip(cnt, elig)]
        assert (got[0][np.isnan(s[0])] == 1).all() and (got[2] == 1).all() and int(n_sel[2]) == 0
    # ties go to the lower row: with count = the -inf rows + 2, the two lowest-indexed rows holding -7 follow the -inf rows
    want_rows = sorted(np.nonzero(np.isinf(s[0]))[0].tolist() + np.nonzero(s[0] == np.float32(-7.0))[0][:2].tolist())
    got_keep, _ = ref.select_lowest(s, (n_inf + 2, 0, 0))
    assert np.nonzero(got_keep[0] == 0)[0].tolist() == want_rows
    # ... and +0.0 / -0.0 tie: the zeros are taken in row order, whatever their sign
    zeros = np.nonzero(s[0] == 0)[0]
    k, _ = ref.select_lowest(s, (below_zero + 4, 0, 0))
    assert np.nonzero((k[0] == 0) & (s[0] == 0))[0].tolist() == zeros[:4].tolist()
    assert len({bool(np.signbit(s[0, z])) for z in zeros[:12]}) == 2              # both signs are among them


def test_select_lowest_refuses_more_rows_than_fit(lib):
    T = 1025
    score = torch.zeros(T)
    c = torch.ones(1, dtype=torch.int32)
    keep_out, n_sel = torch.full((T, ), 9, dtype=torch.uint8), torch.full((1, ), -5, dtype=torch.int32)
    rc = lib.t2h_select_lowest(score.data_ptr(), c.data_ptr(), 1, T, keep_out.data_ptr(), n_sel.data_ptr(), None)
    assert rc != 0 and b'1025' in lib.emu_last_error()
    assert bool((keep_out == 9).all()) and int(n_sel[0]) == -5
    T = 1024                                                                     # the largest that fits
    score = torch.from_numpy(-np.arange(T, dtype=np.float32))
    keep_out = torch.full((T, ), 9, dtype=torch.uint8)
    c[0] = 3
    assert lib.t2h_select_lowest(score.data_ptr(), c.data_ptr(), 1, T, keep_out.data_ptr(), n_sel.data_ptr(), None) == 0
    assert np.nonzero(keep_out.numpy() == 0)[0].tolist() == [T - 3, T - 2, T - 1] and int(n_sel[0]) == 3


@pytest.mark.parametrize('mode', ['improve', 'always'])
def test_accept_merge(lib, mode):
    B, T, H = 5, 15, 3
    n = B * T
    rs = np.random.RandomState(11)
    cand = torch.from_numpy(rs.randint(0, 1024, size=(H, n)).astype(np.int64))
    cur0 = rs.randint(0, 1024, size=(H, n)).astype(np.int64)
    cand_s = torch.from_numpy(rs.standard_normal(n).astype(np.float32))
    cur_s0 = rs.standard_normal(n).astype(np.float32)
    #           greater    equal      smaller    -inf candidate        NaN candidate
    sum_cand = np.array([-10.0, -20.0, -31.0, -np.inf, np.nan], dtype=np.float32)
    sum_cur = np.array([-10.5, -20.0, -30.0, -40.0, -50.0], dtype=np.float32)
    take = ref.accept(sum_cand, sum_cur, mode)
    assert take.tolist() == ([True, False, False, False, False] if mode == 'improve' else [True] * 5)
    wc, cur = _padded(H * n, torch.int64, -12345)
    cur.copy_(torch.from_numpy(cur0.reshape(-1)))
    ws, cur_s = _padded(n, torch.float32, 555.0)
    cur_s.copy_(torch.from_numpy(cur_s0))
    wo, sum_out = _padded(B, torch.float32, 555.0)
    wa, acc = _padded(B, torch.uint8, 0xEE)
    sc, su = torch.from_numpy(sum_cand.copy()), torch.from_numpy(sum_cur.copy())
    rc = lib.t2h_accept_merge(cand.data_ptr(), cand_s.data_ptr(), sc.data_ptr(), su.data_ptr(), int(mode == 'always'),
                              cur.data_ptr(), cur_s.data_ptr(), sum_out.data_ptr(), acc.data_ptr(), B, T, H, None)
    assert rc == 0, lib.emu_last_error()
    rows = np.repeat(take, T)
    assert cur.numpy().reshape(H, n).tobytes() == np.where(rows[None], cand.numpy(), cur0).tobytes()
    assert cur_s.numpy().tobytes() == np.where(rows, cand_s.numpy(), cur_s0).tobytes()
    assert sum_out.numpy().tobytes() == np.where(take, sum_cand, sum_cur).tobytes()
    assert acc.numpy().tolist() == take.astype(np.uint8).tolist()
    assert su.numpy().tobytes() == sum_cur.tobytes()                             # only read
    assert all(_untouched(w, f) for w, f in ((wc, -12345), (ws, 555.0), (wo, 555.0), (wa, 0xEE)))
