"""Per-image seeds on the CPU (csrc/sampler.hip through tests/emu): the batched unmasking schedule
against the single-image entry points it restates, image by image, and the sampling tail with one seed per image
against scalar-seed calls on each image's own rows.  Everything is compared for integer / bit equality: the two sides
run the same device functions, so the emulator's own libm does not enter."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))
sys.path.insert(0, HERE)
import build_emu  # noqa: E402
import per_image_ref as ref  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')

N_HEADS = 18
SEEDS = (2021, (1 << 63) + 12345, 7)   # (one with the top bit set: the seed is a uint64)


@pytest.fixture(scope='module')
def lib():
    from text2human_amd import _lib
    so = build_emu.load('sampler.hip')
    assert so.t2h_unmask_schedule_batch.argtypes == _lib.SIGNATURES['t2h_unmask_schedule_batch'][1]
    return so


def _geometry(T, n_class=1024):
    """ATen's grid and offset increments of a T-element and a T * n_class-element draw on a device with room for both"""
    grid = 256 * ((T + 255) // 256)
    e_grid = 256 * ((T * n_class + 255) // 256)
    return grid, ((T - 1) // (grid * 4) + 1) * 4, ((T * n_class - 1) // (e_grid * 4) + 1) * 4


def _textures(B, T, seed=4):
    g = torch.Generator().manual_seed(seed)
    tex = torch.randint(0, N_HEADS, (B * T, ), generator=g)
    tex[::5] = 17   # (the last head takes part at every size)
    return tex.contiguous()


def _keep(T):
    """image 0 all kept but 3 rows, image 1 none, image 2 every other row"""
    keep = torch.zeros(3, T, dtype=torch.uint8)
    keep[0] = 1
    keep[0, [1, T // 2, T - 1]] = 0
    keep[2, ::2] = 1
    return keep.reshape(-1).contiguous()


def batch_schedule(lib, seeds, tex, keep, B, T, steps):
    grid, rand_inc, expo_inc = _geometry(T)
    sd = np.array([s & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64)
    step = torch.full((B * T, ), -7, dtype=torch.int32)
    mask = torch.full((B, steps + 1), -7, dtype=torch.int32)
    rc = lib.t2h_unmask_schedule_batch(sd.ctypes.data, grid, rand_inc, expo_inc, tex.data_ptr(),
                                       keep.data_ptr() if keep is not None else None, B, T, steps, N_HEADS,
                                       step.data_ptr(), mask.data_ptr(), None)
    assert rc == 0, lib.emu_last_error()
    return step.view(B, T), mask


def single_schedule(lib, seed, tex, keep, T, steps):
    grid, rand_inc, expo_inc = _geometry(T)
    step = torch.full((T, ), -7, dtype=torch.int32)
    mask = torch.full((steps + 1, ), -7, dtype=torch.int32)
    if keep is None:
        rc = lib.t2h_unmask_schedule(seed, 0, grid, rand_inc, expo_inc, tex.data_ptr(), T, steps, N_HEADS, step.data_ptr(),
                                     mask.data_ptr(), None)
    else:
        rc = lib.t2h_unmask_schedule_keep(seed, 0, grid, rand_inc, expo_inc, tex.data_ptr(), keep.data_ptr(), T, steps,
                                          N_HEADS, step.data_ptr(), mask.data_ptr(), None)
    assert rc == 0, lib.emu_last_error()
    return step, mask


@pytest.mark.parametrize('with_keep', [False, True])
@pytest.mark.parametrize('steps', [16, 37])
@pytest.mark.parametrize('T', [16, 24, 512])
def test_batched_schedule_is_every_images_own_single_schedule(lib, T, steps, with_keep):
    B = 3
    tex = _textures(B, T)
    keep = _keep(T) if with_keep else None
    step, mask = batch_schedule(lib, SEEDS, tex, keep, B, T, steps)
    heads_seen = 0
    for b in range(B):
        t_b = tex[b * T:(b + 1) * T].clone()
        k_b = keep[b * T:(b + 1) * T].clone() if with_keep else None
        want_step, want_mask = single_schedule(lib, SEEDS[b], t_b, k_b, T, steps)
        assert torch.equal(step[b], want_step), f'image {b}: step_of_row differs'
        assert torch.equal(mask[b], want_mask), f'image {b}: head_mask differs'
        if with_keep:
            assert torch.equal(step[b] == 0, k_b != 0)   # kept rows: step 0, and only they
        else:
            assert (step[b] >= 1).all() and (step[b] <= steps).all()
        m = 0
        for t in range(steps + 1):
            m |= int(mask[b, t]) & 0xFFFFFFFF
        heads_seen += bin(m).count('1')
        drawn = t_b[step[b] > 0]
        assert m == sum(1 << int(h) for h in set(drawn.tolist()))   # a head bit per texture that is drawn, no other
    assert heads_seen > 3 * (1 if with_keep else 4)   # (the texture ids are spread over several heads)


def test_batched_schedule_of_one_image_is_the_single_entry_point(lib):
    T, steps = 512, 16
    tex = _textures(1, T, seed=9)
    step, mask = batch_schedule(lib, [SEEDS[1]], tex, None, 1, T, steps)
    want_step, want_mask = single_schedule(lib, SEEDS[1], tex, None, T, steps)
    assert torch.equal(step[0], want_step) and torch.equal(mask[0], want_mask)


def test_batched_schedule_depends_on_the_seed_and_on_nothing_else(lib):
    T, steps = 24, 16
    tex = _textures(1, T).repeat(3)   # the same image three times
    step, mask = batch_schedule(lib, [5, 5, 6], tex, None, 3, T, steps)
    assert torch.equal(step[0], step[1]) and torch.equal(mask[0], mask[1])        # same seed, same textures: same schedule
    assert not torch.equal(step[0], step[2])                                      # another seed: another one


def test_batched_schedule_validates_its_arguments(lib):
    T, steps = 16, 16
    tex = _textures(1, T)
    sd = np.array([1], dtype=np.uint64)
    step, mask = torch.zeros(T, dtype=torch.int32), torch.zeros(steps + 1, dtype=torch.int32)
    args = lambda **kw: [kw.get('seeds', sd.ctypes.data), 256, kw.get('rand_inc', 4), 4, tex.data_ptr(), None,
                         kw.get('B', 1), T, kw.get('steps', steps), N_HEADS, step.data_ptr(), mask.data_ptr(), None]
    assert lib.t2h_unmask_schedule_batch(*args()) == 0
    for bad in (dict(seeds=None), dict(B=0), dict(steps=0), dict(steps=4097), dict(rand_inc=3)):
        assert lib.t2h_unmask_schedule_batch(*args(**bad)) != 0, bad


# ---- the tail: at the shapes of test_sampler_emulated.py, three images of 8 rows
N, C, N_CLASS, TAIL_HEADS, T_IMG = 24, 512, 128, 4, 8
GRID = 256 * (T_IMG * N_CLASS // 256)   # one image's [T, n_class] draw


def _tail_problem():
    g = torch.Generator().manual_seed(12)
    hidden = torch.randn(N, C, generator=g) * 1.5 + 0.2
    gamma, beta = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    w = torch.randn(TAIL_HEADS, N_CLASS, C, generator=g) * 0.08
    tex = torch.randint(0, TAIL_HEADS, (N, ), generator=g)
    return hidden, gamma, beta, w, tex


def _tail_call(lib, pb, rows, offs, temp, seed=None, seed_img=None, rng_rows=None, table=None, top_k=0, logp=False,
               set_offsets=True, expect_ok=True):
    """one t2h_sample_heads[_per_sample] call on the two-launch form -> (x_t, out_idx, logp)"""
    from text2human_amd._lib import SampleHeadsArgs
    hidden, gamma, beta, w, tex = pb
    rows_t = torch.tensor(rows, dtype=torch.int32)
    offs_a = np.array(offs, dtype=np.uint64)
    a = SampleHeadsArgs()
    x_t = torch.full((N, ), -5, dtype=torch.int64)
    out = torch.full((TAIL_HEADS, N), -1, dtype=torch.int64)
    lp = torch.full((N, ), float('nan'))
    ws = torch.zeros(len(rows), N_CLASS)
    a.hidden, a.lnf_gamma, a.lnf_beta, a.w_heads = hidden.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr()
    a.rows, a.tex, a.x_t, a.out_idx = rows_t.data_ptr(), tex.data_ptr(), x_t.data_ptr(), out.data_ptr()
    a.temp, a.n_rows, a.n, a.C, a.n_class, a.n_heads = temp, len(rows), N, C, N_CLASS, TAIL_HEADS
    a.logits_ws, a.philox_grid_threads, a.top_k = ws.data_ptr(), GRID, top_k
    if set_offsets:
        a.row_philox_offset = offs_a.ctypes.data
    if logp:
        a.logp = lp.data_ptr()
    keep_alive = []
    if seed_img is not None:
        sd = np.array(seed_img, dtype=np.uint64)
        keep_alive.append(sd)
        a.philox_seed_img, a.img_rows = sd.ctypes.data, T_IMG
        a.philox_seed = 0xDEAD   # (not read)
    else:
        a.philox_seed = seed
    if rng_rows is not None:
        rr = torch.tensor(rng_rows, dtype=torch.int32)
        keep_alive.append(rr)
        a.rng_rows = rr.data_ptr()
    if table is not None:
        rc = lib.t2h_sample_heads_per_sample(ctypes.byref(a), table.data_ptr(), T_IMG, None)
    else:
        rc = lib.t2h_sample_heads(ctypes.byref(a), None)
    if not expect_ok:
        return rc
    assert rc == 0, lib.emu_last_error()
    return x_t, out, lp


# a row list that mixes the three images and several generator offsets (a compact round: every image at its own step)
ROWS = [17, 0, 9, 3, 23, 10, 8, 7, 16]
OFFS = [4 * (100 + 3 * (r // T_IMG) + (r % 3)) for r in ROWS]


@pytest.mark.parametrize('controls', ['plain', 'top-k + table + logp'])
def test_seeded_tail_is_three_scalar_seed_calls(lib, controls):
    pb = _tail_problem()
    if controls == 'plain':
        kw, temp = dict(), 0.9
    else:   # image 0: the defaults inside a truncating launch; 1: colder, top-k; 2: warmer, another top-k
        sets = ref.settings(temp=(1.0, 0.7, 1.3), top_k=(None, 5, 40), top_p=(None, None, None))
        kw, temp = dict(table=torch.from_numpy(ref.table(sets)), logp=True), -1.0   # (temp is not read)
    x_t, out, lp = _tail_call(lib, pb, ROWS, OFFS, temp, seed_img=SEEDS, **kw)
    want_x, want_out, want_lp = torch.full_like(x_t, -5), torch.full_like(out, -1), torch.full_like(lp, float('nan'))
    for b in range(3):
        sel = [i for i, r in enumerate(ROWS) if r // T_IMG == b]
        rows_b = [ROWS[i] for i in sel]
        xb, ob, lb = _tail_call(lib, pb, rows_b, [OFFS[i] for i in sel], temp, seed=SEEDS[b],
                                rng_rows=[r % T_IMG for r in rows_b], **kw)
        idx = torch.tensor(rows_b)
        want_x[idx], want_out[:, idx], want_lp[idx] = xb[idx], ob[:, idx], lb[idx]
        others = torch.ones(N, dtype=torch.bool)
        others[idx] = False
        assert (xb[others] == -5).all()
    assert torch.equal(x_t, want_x) and torch.equal(out, want_out)
    assert torch.equal(lp.view(torch.int32), want_lp.view(torch.int32))   # bit for bit (NaN where no row was listed)
    listed = torch.tensor(ROWS)
    assert (x_t[listed] >= 0).all() and bool(torch.isfinite(lp[listed]).all()) == (controls != 'plain')
    # non-vacuity: the seed of the row's image is what is used -- with the seeds rotated, tokens move
    x_rot, _, _ = _tail_call(lib, pb, ROWS, OFFS, temp, seed_img=SEEDS[1:] + SEEDS[:1], **kw)
    assert not torch.equal(x_rot, x_t)


def test_seeded_tail_explicit_noise_rows_still_win(lib):
    pb = _tail_problem()
    default = _tail_call(lib, pb, ROWS, OFFS, 0.9, seed_img=SEEDS)
    same = _tail_call(lib, pb, ROWS, OFFS, 0.9, seed_img=SEEDS, rng_rows=[r % T_IMG for r in ROWS])
    assert torch.equal(default[0], same[0]) and torch.equal(default[1], same[1])
    moved = _tail_call(lib, pb, ROWS, OFFS, 0.9, seed_img=SEEDS, rng_rows=[(r + 1) % T_IMG for r in ROWS])
    assert not torch.equal(default[0], moved[0])


def test_seeded_tail_needs_per_row_offsets(lib):
    pb = _tail_problem()
    rc = _tail_call(lib, pb, ROWS, OFFS, 0.9, seed_img=SEEDS, set_offsets=False, expect_ok=False)
    assert rc != 0 and b'row_philox_offset' in lib.emu_last_error()
