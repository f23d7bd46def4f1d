"""Per-image seeds, the host surface that needs no GPU: validation of `seeds`, the seed an entry point
derives for an image, the option combinations that must raise, and the host bookkeeping (per-image offsets, the round
plan's local noise rows)."""
import argparse
import hashlib

import numpy as np
import pytest
import torch

from text2human_amd import defaults, options, sample_from_parsing, schedule


def test_seeds_are_validated():
    assert options.image_seeds(3, [0, 5, (1 << 64) - 1]) == [0, 5, (1 << 64) - 1]
    assert options.image_seeds(2, (7, 8)) == [7, 8]
    assert options.image_seeds(2, np.array([1, 1 << 63], dtype=np.uint64)) == [1, 1 << 63]
    assert options.image_seeds(2, torch.tensor([3, 4])) == [3, 4]
    for bad, word in (([1, 2], 'one entry per image'),            # wrong length
                      ([1, 2, 3, 4], 'one entry per image'),
                      ([1, -1, 2], 'image 1'),                    # negative
                      ([1, 2, 1 << 64], 'image 2'),               # >= 2^64
                      ([True, 2, 3], 'image 0'),                  # bool
                      ([1, 2.0, 3], 'image 1'),                   # float
                      (np.array([1.0, 2.0, 3.0]), 'image 0'),
                      (np.array([True, False, True]), 'image 0'),
                      (['1', 2, 3], 'image 0'),
                      (5, 'one integer per image'),               # a scalar is no per-image sequence
                      (None, 'one integer per image')):
        with pytest.raises(ValueError, match=word):
            options.image_seeds(3, bad)


def test_derived_seed_known_answers():
    # first 8 bytes, big-endian, of SHA-256("{manual_seed}:{img_name}")
    assert options.image_seed(2021, 'MEN-Denim-id_00000080-01_7_additional.png') == 1944073210598470632
    assert options.image_seed(7, 'a.png') == 15617916113710196824
    want = int.from_bytes(hashlib.sha256(b'2021:x/y.png').digest()[:8], 'big')
    assert options.image_seed(2021, 'x/y.png') == want and 0 <= want < 1 << 64
    assert options.image_seed(2022, 'x/y.png') != want and options.image_seed(2021, 'x/z.png') != want


def test_derived_seed_does_not_depend_on_the_list_an_image_is_in():
    names = [f'img_{i:03d}.png' for i in range(8)]
    alone = {n: options.image_seed(2021, n) for n in names}
    for batch in (names[:4], names[4:], names[::-1], [names[5]], names[2:7]):
        assert [options.image_seed(2021, n) for n in batch] == [alone[n] for n in batch]
    assert len(set(alone.values())) == len(names)
    assert options.image_seeds(8, [alone[n] for n in names]) == [alone[n] for n in names]   # (valid `seeds`)


def _opt(**kw):
    opt = defaults.with_per_image_seeds(defaults.sample_from_parsing())
    opt.update(kw)
    return opt


def test_option_combinations_that_must_raise():
    assert options.per_image_seeding(_opt()) is True
    assert options.per_image_seeding(defaults.sample_from_parsing()) is False
    assert options.per_image_seeding(defaults.with_per_image_seeds(_opt(), on=False)) is False
    assert options.per_image_seeding(_opt(sample_order='random', sample_best_of=1, sample_top_k=5, sample_top_p=0.9)) is True
    for bad, word in ((dict(sample_order='confidence'), 'sample_order'),
                      (dict(sample_best_of=2), 'sample_best_of'),
                      (dict(refine_temp=0.8), 'refine_temp'),
                      (dict(refine_top_k=5), 'refine_top_k'),
                      (dict(refine_top_p=0.5), 'refine_top_p'),
                      (dict(per_image_seeds='yes'), 'true or false')):
        with pytest.raises(ValueError, match=word):
            options.per_image_seeding(_opt(**bad))
    # without the flag those keys are what they always were
    assert options.per_image_seeding(defaults.with_confidence_order(defaults.sample_from_parsing())) is False


def test_command_line_flag_sets_the_option_and_is_checked_with_the_others():
    ap = sample_from_parsing.cli_parser()
    opt = sample_from_parsing.apply_cli(defaults.sample_from_parsing(), ap.parse_args(['-opt', 'x.yml', '--per-image-seeds']))
    assert opt['per_image_seeds'] is True
    opt = sample_from_parsing.apply_cli(defaults.sample_from_parsing(), ap.parse_args(['-opt', 'x.yml']))
    assert 'per_image_seeds' not in opt
    for extra in (['--order', 'confidence'], ['--best-of', '3'], ['--refine-temp', '0.7']):
        with pytest.raises(ValueError, match='per_image_seeds'):
            sample_from_parsing.apply_cli(defaults.sample_from_parsing(),
                                          ap.parse_args(['-opt', 'x.yml', '--per-image-seeds'] + extra))
    # a namespace of an older caller (no such attribute) is what it always was
    ns = argparse.Namespace(order=None, rounds=None, top_k=None, top_p=None, best_of=None, refine_temp=None,
                            refine_top_k=None, refine_top_p=None)
    assert 'per_image_seeds' not in sample_from_parsing.apply_cli(defaults.sample_from_parsing(), ns)


def test_per_image_offsets_follow_every_images_own_head_mask():
    steps, n_heads, rand_inc, expo_inc = 4, 3, 4, 16
    masks = np.array([[0, 0b001, 0b110, 0, 0b111],      # image 0
                      [0, 0b100, 0, 0, 0b010]])         # image 1
    expo_off, final = schedule.draw_offsets_per_image(masks, steps, rand_inc, expo_inc, n_heads)
    for b in range(2):
        _, want, end = schedule.draw_offsets(masks[b], steps, 0, rand_inc, expo_inc, n_heads)
        assert np.array_equal(expo_off[b], want) and final[b] == end
    assert final.tolist() == [4 * 4 + 6 * 16, 4 * 4 + 2 * 16]
    assert expo_off[1, 4, 1] == 4 and expo_off[0, 4, 1] == 4 + 16 and expo_off[1, 1, 2] == 4 * 4 + 16


@pytest.mark.parametrize('shrink', [False, True])
def test_round_plan_takes_offsets_per_image_and_local_noise_rows(shrink):
    B, T, steps, n_heads = 3, 4, 3, 2
    # image 0 takes one round, image 1 three, image 2 two: with shrink the batch is reordered to [1, 2, 0]
    step_of_row = np.array([2, 2, 2, 2, 3, 2, 1, 1, 3, 3, 1, 1], dtype=np.int32)
    tex = np.array([0, 1, 0, 1, 0, 0, 1, 1, 1, 1, 0, 0])
    expo_off = np.arange(B * (steps + 1) * n_heads, dtype=np.int64).reshape(B, steps + 1, n_heads) * 4
    p = schedule.plan_rounds(step_of_row, tex, B, T, True, shrink, None, expo_off, per_image=True)
    assert (p.perm is not None) == shrink
    if shrink:
        assert p.perm.tolist() == [1, 2, 0]
    perm = np.arange(B) if p.perm is None else p.perm
    assert len(p.order) == B * T
    for i, r in enumerate(p.order):
        img, local = perm[r // T], r % T                 # the caller's image of listed row r, its row there
        orig = img * T + local
        assert p.rng_rows[i] == local                    # the noise row is local, reordered or not
        assert p.offs[i] == expo_off[img, step_of_row[orig], tex[orig]]
    # the scalar form is what it was: one table for the batch, global noise rows only when the batch is reordered
    q = schedule.plan_rounds(step_of_row, tex, B, T, True, shrink, None, expo_off[0])
    assert np.array_equal(q.order, p.order) and (q.rng_rows is None) == (not shrink)
    # the two forms cannot be confused: each refuses the other's table
    with pytest.raises(ValueError):
        schedule.plan_rounds(step_of_row, tex, B, T, True, shrink, None, expo_off)
    with pytest.raises(ValueError):
        schedule.plan_rounds(step_of_row, tex, B, T, True, shrink, None, expo_off[0], per_image=True)
