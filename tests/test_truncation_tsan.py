"""ThreadSanitizer over the row-threshold selection of truncated sampling (csrc/sampler.hip, DESIGN.md "Truncated
sampling"): its LDS histograms are filled by atomics and then read, zeroed and answered through plain LDS accesses of
the first wave -- ordered by the workgroup barrier (workgroup scope) or the wave's own wait (wave scope).  Built and
run like tests/test_lds_races_tsan.py (driver: tests/emu/tsan/sampler.cpp).  The negative control drops the
synchronisation between the atomics and the reads and must be reported."""
import pytest

import test_lds_races_tsan as T

pytestmark = T.pytestmark


def test_selection_has_no_lds_race():
    found = T.races(T.build_driver('sampler'))
    assert not found, found[:3]


def test_a_removed_synchronisation_is_reported():
    def drop_sync(text):
        a = text.index('uint32_t trunc_select(')
        marker = '      trunc_sync<NT>();\n      if (t < 64) {'
        b = text.index(marker, a)
        return text[:b] + '      if (t < 64) {' + text[b + len(marker):]
    found = T.races(T.build_driver('sampler', transform=drop_sync, tag='_no_hist_sync'))
    assert found, 'a missing synchronisation went unnoticed'
