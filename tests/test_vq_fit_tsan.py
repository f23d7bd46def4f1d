"""ThreadSanitizer over the all-codebook fit (csrc/vq_fit.hip): two operand buffers with ONE barrier per K
tile, the code norms handed from the staging threads to the epilogue through LDS, the final merge of the waves of a
row.  Built and run like tests/test_lds_races_tsan.py (driver: tests/emu/tsan/vq_fit.cpp), once per row tile.  The
negative control drops the main loop's barrier and must be reported."""
import pytest

import test_lds_races_tsan as T

pytestmark = T.pytestmark


@pytest.mark.parametrize('tile', [32, 64, 128])
def test_fit_has_no_lds_race(tile):
    found = T.races(T.build_driver('vq_fit'), tile)
    assert not found, found[:3]


def test_a_removed_barrier_is_reported():
    def drop_loop_barrier(text):
        marker = '    __syncthreads();\n  }\n\n  // ---- combine'
        b = text.index(marker)
        return text[:b] + '  }\n\n  // ---- combine' + text[b + len(marker):]
    found = T.races(T.build_driver('vq_fit', transform=drop_loop_barrier, tag='_no_loop_barrier'), 32)
    assert found, 'a missing barrier went unnoticed'
