"""GPU: the exclusive scan u32 -> u64 (sc_scan.hip: launch_scan_u32, launch_scan_u32_pair) in each of its forms, at its edges.

Through tests/native/kernel_probe.hip, against np.cumsum in uint64 (tests/kernel_probe.py), every word: out[0 .. n], the sentinel in
the tiles a range leaves out, the CSR bases, the pinned total — and nothing behind any buffer.  The look-back form is never given a
total of 2^50 or more, a ticket that is not zero or an epoch twice: those are outside its contract (sc_kernels.hpp, LbArgs)."""
import numpy as np
import pytest

import kernel_probe as kp
from kernel_probe import SCAN_TILE, SCAN_SMALL_MAX, u32, u64

pytestmark = pytest.mark.gpu

FORMS = ["lookback", "self", "three"]


def _tiles(n):
    return (n + SCAN_TILE - 1) // SCAN_TILE


def _lb_for(n):
    return kp.LbState(kp.load().kp_scan_temp_bytes(max(n, 1)))


def _check(vals, form, rng_=None, lb=None, epoch=1, extras=True, tag=""):
    n = len(vals)
    if form == "lookback" and lb is None:
        lb = _lb_for(n)
    exp = kp.expect_scan(vals, rng_)
    assert form != "lookback" or int(exp[n]) < kp.LB_VALUE_LIMIT, (tag, "an illegal input: the look-back form carries 50 bits")
    got = kp.run_scan(vals, form, rng_=rng_, lb=lb, epoch=epoch, with_ebase=extras, with_host=True)
    print(tag, "n", n, "tiles", _tiles(n), form, "range", rng_, "total", int(got["out"][n]), "expected", int(exp[n]))
    assert got["ok"], (tag, "a guard behind a buffer, the ticket or the error word was written")
    assert got["input_kept"], tag
    assert np.array_equal(got["out"], exp), (tag, np.flatnonzero(got["out"] != exp)[:8])
    assert got["host"] == int(exp[n]), tag
    if extras:
        if n > SCAN_SMALL_MAX:   # scan_writes_ebase(n)
            assert rng_ is None
            assert np.array_equal(got["ebase"], kp.ref_ebase(exp, got["deg"], got["degp"])), tag
        else:
            assert (got["ebase"] == u32(kp.SENT32)).all(), (tag, "the one-block form writes no CSR bases")
    return got, lb


@pytest.mark.parametrize("n", kp.SCAN_SMALL_LENGTHS)
@pytest.mark.parametrize("kind", ["random", "zero", "ones"])
def test_one_block_form(n, kind):
    for form in FORMS:
        _check(kp.scan_values(kind, n, seed=n, lookback=form == "lookback"), form, tag=kind)


@pytest.mark.parametrize("n", kp.SCAN_TILED_LENGTHS)
@pytest.mark.parametrize("form", FORMS)
def test_tiled_forms_around_the_tile_borders(n, form):
    assert _tiles(n) <= kp.LB_MAX_TILES
    _check(kp.scan_values("random", n, seed=n, lookback=form == "lookback"), form)


@pytest.mark.parametrize("form", FORMS)
def test_all_zero_and_all_ones(form):
    _check(kp.scan_values("zero", 3 * SCAN_TILE + 1), form, tag="zero")
    # 48 tiles of 0xFFFFFFFF: the largest prefixes the look-back's 50-bit value field is asked to carry here
    got, _ = _check(kp.scan_values("ones", kp.ONES_LB_N), form, tag="ones")
    assert int(got["out"][kp.ONES_LB_N]) == 3 * 2 ** 48 - 196608 < 2 ** 50
    if form != "lookback":      # a total past 2^50 is legal without look-back only, and must be exact
        got, _ = _check(kp.scan_values("ones", kp.ONES_BIG_N), form, tag="ones past 2^50")
        assert int(got["out"][kp.ONES_BIG_N]) == 2 ** 52 - 2 ** 20 > 2 ** 50


@pytest.mark.parametrize("tiles,ranged", [(256, False), (257, False), (512, True), (513, True)])
def test_the_switch_between_look_back_and_two_launches(tiles, ranged):
    """LbArgs given on both sides of the limit (256 tiles, 512 with a range): below it the descriptors are written, above it the
    two-launch form runs and leaves them alone.  The result is the same prefix."""
    for n in (tiles * SCAN_TILE, tiles * SCAN_TILE - 1):
        vals = kp.scan_values("random", n, seed=tiles, lookback=True)
        rng_ = (SCAN_TILE + 7, n - 3 * SCAN_TILE - 9) if ranged else None
        got, lb = _check(vals, "lookback", rng_=rng_, extras=not ranged, tag=f"{tiles} tiles")
        desc = lb.desc.read(u64)
        limit = kp.LB_MAX_TILES_RANGE if ranged else kp.LB_MAX_TILES
        if tiles <= limit:
            assert (desc[:tiles] >> u64(52) == u64(1)).all() and (desc[:tiles] >> u64(50) & u64(3) == u64(2)).all()   # epoch 1, inclusive prefixes
        else:
            assert not desc.any()


def test_past_1024_tiles_in_three_launches():
    """scan_self_max = 0 and more than 1024 tiles: the one-block scan of the block sums takes a second trip with a carry."""
    assert _tiles(kp.SCAN_CARRY_LENGTH) > 1024
    _check(kp.scan_values("random", kp.SCAN_CARRY_LENGTH, seed=5), "three", extras=False)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [5 * SCAN_TILE + 777, 6 * SCAN_TILE])
def test_ranges(form, n):
    """Garbage outside [lo, hi): it counts as zero without being summed, the tiles wholly outside keep the sentinel in `out`, out[n]
    is the total."""
    vals = kp.scan_values("random", n, seed=n, lookback=form == "lookback")
    for name, rng_ in kp.scan_ranges(n).items():
        got, _ = _check(vals, form, rng_=rng_, extras=False, tag=name)
        dead = kp.scan_dead_tiles(n, rng_)
        if name in ("empty", "empty_front"):
            assert len(dead) == _tiles(n) and int(got["out"][n]) == 0
        if name == "last_tile":
            assert dead == list(range(_tiles(n) - 1))
        if name == "borders":
            assert dead == [0] + list(range(3, _tiles(n)))


@pytest.mark.parametrize("n", [SCAN_SMALL_MAX - 1, SCAN_SMALL_MAX, SCAN_SMALL_MAX + 1, 3 * SCAN_TILE + 5])
@pytest.mark.parametrize("second", [True, False])
@pytest.mark.parametrize("self_max", [-1, 0])
def test_the_pair_call(n, second, self_max):
    L = kp.load()
    a, b = kp.scan_values("random", n, seed=1), kp.scan_values("random", n, seed=2)
    d_a, d_b = kp.DevBuf.of(a), kp.DevBuf.of(b)
    o_a, o_b = kp.DevBuf((n + 1) * 8), kp.DevBuf((n + 1) * 8)
    tb = L.kp_scan_temp_bytes(n)
    tmp, host = kp.DevBuf(tb), kp.Pinned()
    rc = L.kp_scan_pair(d_a.ptr, o_a.ptr, d_b.ptr if second else None, o_b.ptr if second else None, n, tmp.ptr, tb, self_max, host.ptr, kp.stream())
    assert rc == 0
    kp.sync()
    assert np.array_equal(o_a.read(u64), kp.ref_scan(a))
    assert host.get() == int(kp.ref_scan(a)[n])       # array a's total, never b's
    if second:
        assert np.array_equal(o_b.read(u64), kp.ref_scan(b))
    else:
        assert (o_b.read(u64) == u64(kp.SENT64)).all()
    assert all(x.guard_ok() for x in (d_a, d_b, o_a, o_b, tmp))


def test_one_descriptor_area_through_the_epochs():
    """No memset between launches: epochs 1, 2, 3 on one area with 200, 3 and 200 tiles (words of an older epoch under a newer
    launch, at the same and at other tile counts), on to epoch 4095 — then the caller's zeroing and epoch 1 again, as lb_next does."""
    big, small = 200 * SCAN_TILE - 17, 3 * SCAN_TILE - 5
    lb = _lb_for(big)
    plan = [(1, big), (2, small), (3, big), (4, small), (5, big), (4094, big), (4095, big)]
    for epoch, n in plan:
        _check(kp.scan_values("random", n, seed=epoch, lookback=True), "lookback", lb=lb, epoch=epoch, tag=f"epoch {epoch}")
    desc = lb.desc.read(u64)
    assert (desc[:200] >> u64(52) == u64(4095)).all()
    lb.zero_desc()
    for epoch, n in [(1, big), (2, small), (3, big)]:
        _check(kp.scan_values("random", n, seed=100 + epoch, lookback=True), "lookback", lb=lb, epoch=epoch, tag=f"after the wrap, epoch {epoch}")
