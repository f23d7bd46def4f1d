"""The region-editing kernels of csrc/sampler.hip on the CPU (tests/emu): the unmasking schedule started from kept rows
(t2h_unmask_schedule_keep) against a numpy restatement of the reference's loop with `unmasked = keep`, its keep-all-zero
case against t2h_unmask_schedule bit for bit, and the prefill / region -> keep / bottom-index merge kernels against
their numpy statements ("Editing a region")."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import build_emu  # noqa: E402
from test_sampler_emulated import raw_words, uniform_of  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')


@pytest.fixture(scope='module')
def lib():
    return build_emu.load('sampler.hip')


def _loop_with_keep(seed, offset, grid, rand_inc, expo_inc, tex, keep, steps):
    """models/sample_model.py:279-306 with the initial state unmasked = keep: (step_of_row, head_mask, final offset)"""
    n = tex.size
    unmasked = keep.astype(bool).copy()
    step = np.zeros(n, dtype=np.int32)
    mask = np.zeros(steps + 1, dtype=np.uint32)
    off = offset
    for t in range(steps, 0, -1):
        r = uniform_of(raw_words(seed, off, grid, n))
        change = (r < np.float32(1.0) / np.float32(t)) & ~unmasked
        unmasked |= change
        step[change] = t
        heads = np.unique(tex[change])
        mask[t] = sum(1 << int(h) for h in heads)
        off += rand_inc + len(heads) * expo_inc
    return step, mask, off


def _run_keep(lib, seed, offset, grid, rand_inc, expo_inc, tex, keep, steps, n_heads=18):
    n = tex.numel()
    step = torch.full((n, ), -1, dtype=torch.int32)
    mask = torch.zeros(steps + 1, dtype=torch.int32)
    rc = lib.t2h_unmask_schedule_keep(seed, offset, grid, rand_inc, expo_inc, tex.data_ptr(), keep.data_ptr(), n, steps,
                                      n_heads, step.data_ptr(), mask.data_ptr(), None)
    assert rc == 0, lib.emu_last_error()
    return step.numpy(), mask.numpy().view(np.uint32)


@pytest.mark.parametrize('seed,offset,density,steps', [(2021, 40, 0.25, 24), (7, 4 * 1001, 0.5, 17),
                                                        (0x1234567890ABCDEF, 1 << 34, 0.875, 30), (3, 0, 1.0, 9)])
def test_keep_schedule_is_the_loop_started_from_the_kept_rows(lib, seed, offset, density, steps):
    n, grid, rand_inc, expo_inc = 2 * 512, 1024, 4, 4 * 1024
    g = torch.Generator().manual_seed(seed & 0xFFFF)
    tex = torch.randint(0, 18, (n, ), generator=g)
    keep = (torch.rand(n, generator=g) < density).to(torch.uint8)
    step, mask = _run_keep(lib, seed, offset, grid, rand_inc, expo_inc, tex, keep, steps)
    want_step, want_mask, _ = _loop_with_keep(seed, offset, grid, rand_inc, expo_inc, tex.numpy(), keep.numpy(), steps)
    assert np.array_equal(step, want_step) and np.array_equal(mask, want_mask)
    kept = keep.numpy().astype(bool)
    assert (step[kept] == 0).all() and (step[~kept] >= 1).all()     # kept rows: no step; every other row: one
    if density == 1.0:
        assert (mask == 0).all()                                     # nothing drawn: the offset moves by steps * rand_inc


def test_keep_all_zero_is_the_plain_schedule_bit_for_bit(lib):
    n, steps, seed, offset, grid = 3 * 512, 40, 99, 4 * 12, 256 * 6
    tex = torch.randint(0, 18, (n, ), generator=torch.Generator().manual_seed(1))
    step, mask = _run_keep(lib, seed, offset, grid, 4, 4096, tex, torch.zeros(n, dtype=torch.uint8), steps)
    s0 = torch.full((n, ), -1, dtype=torch.int32)
    m0 = torch.zeros(steps + 1, dtype=torch.int32)
    assert lib.t2h_unmask_schedule(seed, offset, grid, 4, 4096, tex.data_ptr(), n, steps, 18, s0.data_ptr(),
                                   m0.data_ptr(), None) == 0, lib.emu_last_error()
    assert np.array_equal(step, s0.numpy()) and np.array_equal(mask, m0.numpy().view(np.uint32))


def _lists(B, T, n_heads, n_class, seed):
    g = torch.Generator().manual_seed(seed)
    tex = torch.randint(0, n_heads, (B * T, ), generator=g)
    src = torch.full((n_heads, B * T), -1, dtype=torch.int64)
    src[tex, torch.arange(B * T)] = torch.randint(0, n_class, (B * T, ), generator=g)
    return tex, src, g


def _prefill(lib, src, tex, keep, mask_id, n_class, check_only=False):
    n_heads, n = src.shape
    x_t = torch.full((n, ), -7, dtype=torch.int64)
    out = torch.full((n_heads, n), -7, dtype=torch.int64)
    err = torch.zeros(1, dtype=torch.int32)
    rc = lib.t2h_edit_prefill(src.data_ptr(), tex.data_ptr(), keep.data_ptr(), mask_id,
                              None if check_only else x_t.data_ptr(), None if check_only else out.data_ptr(),
                              err.data_ptr(), n, n_heads, n_class, None)
    assert rc == 0, lib.emu_last_error()
    return x_t, out, int(err[0])


def test_prefill_is_the_specified_initial_state(lib):
    B, T, H, V = 2, 512, 18, 1024
    tex, src, g = _lists(B, T, H, V, seed=5)
    src[(tex + 3) % H, torch.arange(B * T)] = 17            # entries under OTHER textures: never read
    keep = (torch.rand(B * T, generator=g) < 0.4).to(torch.uint8)
    x_t, out, err = _prefill(lib, src, tex, keep, 18432, V)
    k = keep.bool()
    own = src[tex, torch.arange(B * T)]
    assert err == 0
    assert torch.equal(x_t, torch.where(k, own + V * tex, torch.full_like(own, 18432)))
    want = torch.full((H, B * T), -1, dtype=torch.int64)
    want[tex[k], torch.arange(B * T)[k]] = own[k]
    assert torch.equal(out, want)


def test_prefill_error_word_names_the_first_invalid_kept_row(lib):
    B, T, H, V = 2, 512, 18, 1024
    tex, src, _ = _lists(B, T, H, V, seed=6)
    keep = torch.zeros(B * T, dtype=torch.uint8)
    keep[100:900] = 1
    n = B * T
    assert _prefill(lib, src, tex, keep, 18432, V, check_only=True)[2] == 0
    src[tex[700], 700] = -1                                   # no index under its texture
    src[tex[333], 333] = V                                    # outside the codebook
    src[tex[50], 50] = -1                                     # not kept: no error
    _, _, err = _prefill(lib, src, tex, keep, 18432, V)
    assert err == n - 333
    src[tex[333], 333] = 5
    assert _prefill(lib, src, tex, keep, 18432, V, check_only=True)[2] == n - 700


def _cells_any(region, th, tw):
    """[B, H, W] bool -> [B, th * tw] bool: any pixel of the cell"""
    B, H, W = region.shape
    return region.reshape(B, th, H // th, tw, W // tw).any(4).any(2).reshape(B, th * tw)


@pytest.mark.parametrize('H,W', [(512, 256), (256, 128)])
def test_region_keep_is_an_any_pixel_reduction_per_cell(lib, H, W):
    B, th, tw = 2, 32, 16
    g = torch.Generator().manual_seed(H)
    segm = torch.randint(0, 24, (B, 1, H // 8, W // 8), generator=g).repeat_interleave(8, 2).repeat_interleave(8, 3)
    segm[0, 0, 37, 101] = 23                                  # single pixels: their cells must be caught
    segm[1, 0, H - 1, W - 1] = 22
    segm_f = segm.float().contiguous()
    labels = [5, 22, 23]
    keep = torch.full((B, th * tw), 9, dtype=torch.uint8)
    bits = sum(1 << lb for lb in labels)
    assert lib.t2h_region_keep(None, segm_f.data_ptr(), bits, 2, B, H, W, th, tw, keep.data_ptr(), None) == 0, \
        lib.emu_last_error()
    in_region = torch.isin(segm[:, 0], torch.tensor(labels))
    want = (~_cells_any(in_region, th, tw)).to(torch.uint8)
    assert torch.equal(keep, want) and 0 < int(want.sum()) < B * th * tw
    # pixel masks: uint8 and fp32 (nonzero = edit)
    m = (torch.rand(B, 1, H, W, generator=g) < 0.002)
    for mode, t in ((0, m.to(torch.uint8)), (1, m.float() * 0.5)):
        keep.fill_(9)
        ptrs = (t.data_ptr(), None) if mode == 0 else (None, t.data_ptr())
        assert lib.t2h_region_keep(*ptrs, 0, mode, B, H, W, th, tw, keep.data_ptr(), None) == 0, lib.emu_last_error()
        assert torch.equal(keep, (~_cells_any(m[:, 0], th, tw)).to(torch.uint8)), mode


def test_merge_kept_indices_copies_the_kept_columns(lib):
    H, n = 18, 2 * 512
    g = torch.Generator().manual_seed(8)
    src = torch.randint(-1, 512, (H, n), generator=g)
    dst = torch.randint(-1, 512, (H, n), generator=g)
    keep = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
    want = torch.where(keep.bool()[None, :], src, dst)
    assert lib.t2h_merge_kept_indices(src.data_ptr(), keep.data_ptr(), dst.data_ptr(), n, H, None) == 0
    assert torch.equal(dst, want)
