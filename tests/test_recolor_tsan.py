"""csrc/recolor.hip under ThreadSanitizer on the host emulator (a stand-alone program, tests/emu/tsan/recolor.cpp, built
by the helper of tests/test_lds_races_tsan.py): the staging of the membership codes and of the classification word, and
the hand-off between the horizontal and the vertical integer pass, must be ordered by barriers, at the narrowest and
the widest feather; the negative control drops the barrier between the two passes and must be reported."""
import pytest

import test_lds_races_tsan as T

pytestmark = pytest.mark.skipif(not T._tsan_available(), reason='no host clang++ with ThreadSanitizer')


@pytest.mark.parametrize('feather', [0, 8])
def test_no_lds_race(feather):
    found = T.races(T.build_driver('recolor'), feather)
    assert not found, found[:3]


def test_a_removed_barrier_is_reported():
    def drop_pass_barrier(text):
        marker = '    __syncthreads();\n    // vertical pass'
        assert text.count(marker) == 1
        return text.replace(marker, '    // vertical pass')
    found = T.races(T.build_driver('recolor', transform=drop_pass_barrier, tag='_no_pass_barrier'), 8)
    assert found, 'a missing barrier went unnoticed'
