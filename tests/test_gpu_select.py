"""GPU: stage B's radix select and ordinal-order compaction (sc_tri.hip: launch_select_rounds, launch_compact_count,
launch_compact_write, with launch_scan_u32_pair where the write kernel does not sum the tile counts itself), in the library's own
sequence, through tests/native/kernel_probe.hip.

Expected: the definition (tests/kernel_probe.py ref_select) — order the keys by (key descending, ordinal ascending), take the first
want_eff; kstar is the last key taken, need_eq how many taken keys equal it; the output is the taken ordinals ascending with their
keys.  Every word is compared, nothing may land behind the selection's count, all three histograms are zero again afterwards, and a
second select on the state the first one left gives the same.  Keys are >= 1 throughout (0 is "no key")."""
import numpy as np
import pytest

import kernel_probe as kp
from kernel_probe import CP_TILE, u32, u64

pytestmark = pytest.mark.gpu

KINDS = ["random32", "one_value", "adjacent", "fp32", "fp32_floor"]


def _wants(keys, kmin, M):
    """1, a middle one, M, more than M (clipped) — and around the middle one's k*: exactly the keys above it (need_eq at its upper end:
    the next key value up is taken whole), one more (need_eq == 1), and all of k*'s copies (need_eq == all of them)."""
    mid = M // 2 + 1
    want_eff, kstar, need_eq, _, _ = kp.ref_select(keys, kmin, mid)
    wants = {1, mid, M, M + 7}
    if want_eff:
        above = int((keys > u32(kstar)).sum())
        wants |= {above + 1, above + int((keys == u32(kstar)).sum())}
        if above:
            wants.add(above)
    return sorted(wants)


@pytest.mark.parametrize("M", kp.SELECT_LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_key_patterns_and_lengths(M, kind):
    keys, preset, kmin, kmax, rounds = kp.select_keys(kind, M, seed=M)
    assert keys.min() >= 1
    buf = kp.DevBuf.of(keys)
    for want in _wants(keys, kmin, M):
        kp.select_twice(buf, M, keys, tag=f"{kind} M {M} want {want}", kmin=kmin, kmax=kmax, preset=preset, want=want, rounds=rounds)
    assert np.array_equal(buf.read(u32), keys)


@pytest.mark.parametrize("sel_blocks", [2, 256])
def test_trip_ends_of_the_select_rounds(sel_blocks):
    """M / 4 one below, on and above four and eight grid strides: the last trip of the four-deep loop, the first of the remainder
    loop, and neither.  A wrong trip count drops or doubles keys in a histogram: k* or need_eq move."""
    for M in kp.trip_end_lengths(sel_blocks) + [kp.trip_end_lengths(sel_blocks)[4] + 3]:     # ... and one with a tail of three
        for kind in ("random32", "fp32"):
            keys, preset, kmin, kmax, rounds = kp.select_keys(kind, M, seed=M)
            buf = kp.DevBuf.of(keys)
            for want in ((1000, M - 1) if kind == "fp32" else (1000,)):
                got = kp.run_select(buf, M, kmin=kmin, kmax=kmax, preset=preset, want=want, rounds=rounds, sel_blocks=sel_blocks)
                kp.check_select(got, keys, kmin, want, tag=f"sel_blocks {sel_blocks} M {M} {kind} want {want}")


@pytest.mark.parametrize("name", list(kp.TIE_BLOCKS))
@pytest.mark.parametrize("self_max", [-1, 0])
def test_the_cut_among_equal_keys(name, self_max):
    """A block of keys == k* across one, two and many tile borders of the compaction, the cut on the last entry of a tile, on the first
    of the next and in the middle: the first need_eq of them by ordinal are taken, no other."""
    M, a, b, cut, n_above = kp.TIE_BLOCKS[name]
    keys, want = kp.tie_case(name)
    buf = kp.DevBuf.of(keys)
    got, n = kp.select_twice(buf, M, keys, tag=name, kmin=int(keys.min()), kmax=int(keys.max()), preset=0, want=want, rounds=3, compact_self_max=self_max)
    assert got["self_summed"] == (1 if self_max < 0 else 0)
    assert got["kstar"] == kp.SELECT_KSTAR and got["need_eq"] == cut - a + 1 and n == want
    taken_eq = got["ord"][:n][got["key"][:n] == u32(kp.SELECT_KSTAR)]
    assert np.array_equal(taken_eq, np.arange(a, cut + 1, dtype=u64))


def test_the_scanned_compaction():
    """Past compact_self_max = 4096 tiles the tile counts are scanned by launch_scan_u32_pair; the same form forced at a small M."""
    M = kp.SCANNED_M
    assert kp.load().kp_compact_blocks(M) > 4096
    keys, preset, kmin, kmax, rounds = kp.select_keys("fp32", M, seed=3)
    buf = kp.DevBuf.of(keys)
    for want in (5000, 1):
        got = kp.run_select(buf, M, kmin=kmin, kmax=kmax, preset=preset, want=want, rounds=rounds)
        assert got["self_summed"] == 0
        kp.check_select(got, keys, kmin, want, tag=f"M {M} want {want}")
    M = 5 * CP_TILE + 3
    keys, preset, kmin, kmax, rounds = kp.select_keys("random32", M, seed=4)
    buf = kp.DevBuf.of(keys)
    for self_max, summed in ((0, 0), (-1, 1), (5, 0), (6, 1)):     # 6 tiles: on both sides of the knob
        got = kp.run_select(buf, M, kmin=kmin, kmax=kmax, preset=preset, want=777, rounds=rounds, compact_self_max=self_max)
        assert got["self_summed"] == summed
        kp.check_select(got, keys, kmin, 777, tag=f"compact_self_max {self_max}")


def test_floor_and_shortfall():
    M = 3 * CP_TILE + 2
    keys, preset, _, kmax, rounds = kp.select_keys("fp32", M, seed=9)
    keys[keys > np.float32(2.5).view(u32)] = np.float32(2.25).view(u32)        # nothing above 2.5
    buf = kp.DevBuf.of(keys)
    f = lambda x: int(np.float32(x).view(u32))
    # a floor with no key at or above it: the selection is empty and want is 0
    got = kp.run_select(buf, M, kmin=f(2.75), kmax=kmax, preset=1, want=100, rounds=rounds)
    assert kp.check_select(got, keys, f(2.75), 100, tag="floor above every key") == 0 and got["want"] == 0 and got["short"] == 0
    # the bound promised want_req keys at or above the floor
    there = int((keys >= u32(f(2.4))).sum())
    assert 0 < there < M
    for want, short in ((there + 1, 1), (there, 0), (there - 1, 0), (M, 1)):
        got = kp.run_select(buf, M, kmin=f(2.4), kmax=kmax, preset=1, want=want, want_req=want, rounds=rounds)
        assert kp.check_select(got, keys, f(2.4), want, tag=f"want_req {want} of {there}") == min(want, there)
        assert got["short"] == short, (want, there)
    # ... and with no promise the word stays 0 however few there are
    got = kp.run_select(buf, M, kmin=f(2.4), kmax=kmax, preset=1, want=M, rounds=rounds)
    assert got["short"] == 0


@pytest.mark.parametrize("segments,seg_len", kp.SEGMENT_SHAPES)
def test_segmented_views(segments, seg_len):
    """valid counts 0, 1, 2, 3, 5, seg_len - 1 and seg_len in every position, garbage behind them: the selection of the plain
    concatenation of the valid parts, with ordinals in the view's logical positions."""
    seen = set()
    for seed in range(len(kp.segment_valids(seg_len))):
        store, seg_stride, valid = kp.segmented_case(segments, seg_len, seed=seed)
        seen |= set(valid)
        logical = kp.logical_keys(store, seg_len, seg_stride, valid)
        real = logical[logical != 0]
        assert real.size == sum(valid) and real.min() >= 1
        buf, d_valid = kp.DevBuf.of(store), kp.DevBuf.of(np.asarray(valid, u64))
        M = segments * seg_len
        # the plain concatenation gives the same keys in the same order: its ordinals map to the logical positions
        _, _, _, sel_plain, _ = kp.ref_select(real, 1, real.size // 2 + 1)
        _, _, _, sel_view, _ = kp.ref_select(logical, 1, real.size // 2 + 1)
        assert np.array_equal(np.flatnonzero(logical)[sel_plain.astype(np.int64)], sel_view.astype(np.int64))
        for preset, kmin, kmax, rounds in ((1, kp.F2, kp.F3, 2), (0, int(real.min()), int(real.max()), 3)):
            for want in sorted({1, real.size // 2 + 1, real.size, real.size + 5}):
                kp.select_twice(buf, M, logical, tag=f"{segments} x {seg_len} valid {valid} preset {preset} want {want}", kmin=kmin, kmax=kmax,
                                preset=preset, want=want, rounds=rounds, seg=(seg_len, seg_stride, d_valid))
        assert np.array_equal(buf.read(u32), store) and d_valid.guard_ok()
    assert seen == set(kp.segment_valids(seg_len))
