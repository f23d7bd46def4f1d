"""csrc/composite.hip under ThreadSanitizer on the host emulator (a stand-alone program, tests/emu/tsan/composite.cpp,
built by the helper of tests/test_lds_races_tsan.py): the keep window that borrows the halo buffer, and the hand-off of
the halo and the horizontal pass's buffer between the blur passes of three channels, must be ordered by barriers; the
negative control drops the barrier between the horizontal and the vertical pass and must be reported."""
import pytest

import test_lds_races_tsan as T

pytestmark = pytest.mark.skipif(not T._tsan_available(), reason='no host clang++ with ThreadSanitizer')


@pytest.mark.parametrize('r_lo', [32, 64])
def test_no_lds_race(r_lo):
    found = T.races(T.build_driver('composite'), r_lo)
    assert not found, found[:3]


def test_a_removed_barrier_is_reported():
    def drop_pass_barrier(text):
        marker = '    __syncthreads();\n    // vertical pass'
        assert text.count(marker) == 1
        return text.replace(marker, '    // vertical pass')
    found = T.races(T.build_driver('composite', transform=drop_pass_barrier, tag='_no_pass_barrier'), 32)
    assert found, 'a missing barrier went unnoticed'
