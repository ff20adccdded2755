"""replay.ring_spans, the one place where a write into the replay ring is split at the wrap,
against the slot of every item written out: (at + i) % cap.  No GPU."""
import numpy as np
import pytest

from replay import ring_spans


@pytest.mark.parametrize("at,n,cap", [
    (1, 3, 8),    # no wrap
    (5, 3, 8),    # ends exactly at the end of the ring: at + n == cap
    (6, 5, 8),    # wraps
    (3, 8, 8),    # the whole ring, from the middle
    (0, 8, 8),    # the whole ring, from slot 0
    (7, 1, 8),    # one item in the last slot
    (0, 1, 1),    # a ring of one slot
], ids=lambda v: str(v))
def test_ring_spans_place_every_item_in_its_slot(at, n, cap):
    spans = ring_spans(at, n, cap)
    assert 1 <= len(spans) <= 2
    slot_of = np.full(n, -1)
    for lo, hi, dst in spans:
        assert 0 <= lo < hi <= n and 0 <= dst and dst + (hi - lo) <= cap     # non-empty, inside the ring
        assert (slot_of[lo:hi] == -1).all()                                    # every item once
        slot_of[lo:hi] = np.arange(dst, dst + hi - lo)
    assert slot_of.tolist() == [(at + i) % cap for i in range(n)] == (np.arange(at, at + n) % cap).tolist()
    assert (len(spans) == 2) == (at + n > cap)                                 # two spans only where it wraps
