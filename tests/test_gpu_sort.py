"""GPU: the radix sort of the ranked-list hook (sc_sort.hip, launch_sort_u64) at its tile borders and on both sides of its histogram
scan's one-block limit, through tests/native/kernel_probe.hip.  Expected: the stable sort of the high halves (tests/kernel_probe.py),
every word; the low halves are always the positions, so stability is visible in them."""
import numpy as np
import pytest

import kernel_probe as kp
from kernel_probe import u64

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", kp.SORT_LENGTHS)
def test_sort_equals_the_stable_sort(n):
    L = kp.load()
    tb = L.kp_sort_temp_bytes(n)
    for pattern in kp.SORT_PATTERNS:
        words = kp.sort_words(pattern, n, seed=n)
        d_in, d_out, tmp = kp.DevBuf.of(words), kp.DevBuf(n * 8), kp.DevBuf(tb)
        assert L.kp_sort(d_in.ptr, d_out.ptr, n, tmp.ptr, tb, kp.stream()) == 0
        kp.sync()
        got, exp = d_out.read(u64), kp.ref_sort(words)
        print(pattern, n, "first differing word", np.flatnonzero(got != exp)[:1])
        assert np.array_equal(got, exp), pattern
        if pattern == "equal":
            assert np.array_equal(got, words)       # stability: the output is the input
        assert np.array_equal(d_in.read(u64), words) and d_in.guard_ok() and d_out.guard_ok() and tmp.guard_ok(), pattern
