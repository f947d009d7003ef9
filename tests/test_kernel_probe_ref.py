"""CPU suite for the kernel-level probe (tests/kernel_probe.py, tests/native/kernel_probe.hip): no GPU.

The probe builds here (hipcc cross-compiles) and exports every wrapper; the numpy references agree with brute-force definitions on
tiny inputs; and the case tables of the GPU tests are what they are used for — the tile sizes they are placed by are the sources',
the tie blocks straddle the borders they are named for, the all-ones totals are the stated numbers, the seven match sets differ per
tile, every key array stays >= 1 and the trip-end lengths follow from launch_select_rounds' own formula."""
import os
import re

import numpy as np
import pytest

import kernel_probe as kp
import match_ref
from kernel_probe import CP_TILE, SCAN_TILE, u32, u64

CSRC = os.path.join(kp.PKG_DIR, "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, name
    return m.group(1).strip()


# ---- the probe ------------------------------------------------------------------------------------------------------------------
def test_the_probe_builds_and_exports_every_wrapper(pkg):
    L = kp.load()
    assert os.path.exists(kp.PROBE)
    for name in kp.EXPORTS:
        assert hasattr(L, name), name
    with open(kp.SRC) as f:
        text = f.read()
    assert "__global__" not in text and "<<<" not in text and "hipLaunchKernelGGL" not in text, "the probe holds no kernel of its own"
    assert set(re.findall(r"\b(kp_\w+)\(", text)) == set(kp.EXPORTS)
    # the size helpers are the library's
    for n in (0, 1, SCAN_TILE, SCAN_TILE + 1, 10 ** 6):
        assert L.kp_scan_temp_bytes(n) == ((n + SCAN_TILE - 1) // SCAN_TILE + 4) * 8
        assert L.kp_compact_blocks(n) == (n + CP_TILE - 1) // CP_TILE
    for n in (1, 32, 33, 8192):
        assert L.kp_row_stats_scan_state_bytes(n) == 16 * ((n + kp.RS_ROWS - 1) // kp.RS_ROWS)
    assert L.kp_sort_temp_bytes(0) == 0 and L.kp_sort_temp_bytes(65537) > 65537 * 8
    assert L.kp_select_state_bytes() > 3 * 4096 * 4 and L.kp_select_scratch_bytes(5 * CP_TILE) >= 2 * 5 * 4 + 2 * 6 * 8
    # too little scratch is refused before anything is launched (no GPU is touched)
    assert L.kp_scan(None, 10 ** 6, None, None, 8, -1, None, None, None, 0, None, None, None, None, None, None) == kp.KP_ESCRATCH
    assert L.kp_sort(None, None, 1000, None, 8, None) == kp.KP_ESCRATCH


def test_the_staleness_rule_and_the_missing_compiler(pkg, monkeypatch):
    b = kp._build_module()
    deps = kp.probe_deps(b)
    assert kp.SRC in deps and b.LIB in deps and all(os.path.join(b.CSRC, h) in deps for h in b.HEADERS)
    kp.build_probe()
    assert not b._stale(kp.PROBE, deps)
    monkeypatch.setenv("HIPCC", "/nonexistent/hipcc")
    assert kp.build_probe() == kp.PROBE                      # fresh: no compiler needed
    with pytest.raises(RuntimeError, match="no hipcc"):      # stale and no compiler: an error with a message, not a skip
        kp.build_probe(force=True)


def test_the_tile_sizes_are_the_sources():
    scan, sort, rows, tri = _src("sc_scan.hip"), _src("sc_sort.hip"), _src("sc_rows.hip"), _src("sc_tri.hip")
    assert int(_const(scan, "SCAN_THREADS")) * int(_const(scan, "SCAN_ITEMS")) == SCAN_TILE
    assert int(_const(scan, "SCAN_SMALL_MAX")) == kp.SCAN_SMALL_MAX
    assert f"range ? {kp.LB_MAX_TILES_RANGE} : {kp.LB_MAX_TILES}" in scan          # the form switch of launch_scan_u32
    assert "b0 += 1024" in scan                                                     # scan_of_sums_kernel's trip
    assert int(_const(sort, "RS_TILE")) == kp.RS_TILE
    assert int(_const(rows, "RS_ROWS")) == kp.RS_ROWS
    assert int(_const(tri, "CP_THREADS")) * int(_const(tri, "CP_ITEMS")) == CP_TILE
    assert (int(_const(tri, "SEL_THREADS")), int(_const(tri, "SEL_ITEMS"))) == (kp.SEL_THREADS, kp.SEL_ITEMS)
    assert "uint64_t cap = 256;" in tri and "if (tn.sel_blocks >= 1) cap = tn.sel_blocks;" in tri     # select_grid's rule
    assert int(_const(_src("sc_match.hip"), "FIN_THREADS")) == kp.FIN_TILE
    assert "size_t compact_self_max = 4096;" in _src("sc_kernels.hpp")


# ---- references against brute force -----------------------------------------------------------------------------------------------
def test_scan_reference():
    v = kp.scan_values("random", 37, seed=1)
    exp, run = [], 0
    for x in v.tolist():
        exp.append(run); run += x
    assert kp.ref_scan(v).tolist() == exp + [run]
    lo, hi = 5, 20
    exp, run = [], 0
    for i, x in enumerate(v.tolist()):
        exp.append(run); run += x if lo <= i < hi else 0
    assert kp.ref_scan(v, (lo, hi)).tolist() == exp + [run]
    assert kp.ref_scan(np.zeros(0, u32)).tolist() == [0]
    assert kp.scan_dead_tiles(5 * SCAN_TILE + 1, (SCAN_TILE, 3 * SCAN_TILE)) == [0, 3, 4, 5]
    assert kp.scan_dead_tiles(3 * SCAN_TILE, (SCAN_TILE + 1, SCAN_TILE + 2)) == [0, 2]
    out = kp.ref_scan(v)
    deg, degp = np.arange(37, dtype=u32) * u32(3) + u32(2 ** 31), np.arange(37, dtype=u32)
    assert kp.ref_ebase(out, deg, degp).tolist() == [((o & 0xFFFFFFFF) - (int(a) - int(b))) % 2 ** 32 for o, a, b in zip(out.tolist(), deg, degp)]
    big = kp.expect_scan(kp.scan_values("ones", 3 * SCAN_TILE), (0, SCAN_TILE))
    assert int(big[SCAN_TILE - 1]) == (SCAN_TILE - 1) * kp.ALL_ONES and (big[SCAN_TILE:3 * SCAN_TILE] == u64(kp.SENT64)).all()
    assert int(big[-1]) == SCAN_TILE * kp.ALL_ONES          # out[n] is still the total


def test_sort_reference():
    for pattern in kp.SORT_PATTERNS:
        w = kp.sort_words(pattern, 300, seed=2)
        assert (w & u64(0xFFFFFFFF)).tolist() == list(range(300))          # the low halves are the positions
        exp = sorted(w.tolist(), key=lambda x: x >> 32)                     # Python's sort is stable
        assert kp.ref_sort(w).tolist() == exp == sorted(w.tolist())         # ... and the stable sort of the high halves IS the 64-bit sort
    hi = lambda p: kp.sort_words(p, 5000, 3) >> u64(32)
    assert len(set((hi("top_byte") & u64(0x00FFFFFF)).tolist())) == 1 and len(set((hi("top_byte") >> u64(24)).tolist())) > 200
    assert len(set((hi("low_byte") >> u64(8)).tolist())) == 1 and len(set((hi("low_byte") & u64(255)).tolist())) > 200
    assert len(set(hi("two").tolist())) == 2 and len(set(hi("equal").tolist())) == 1 and (np.diff(hi("descending").astype(np.int64)) <= 0).all()
    cells = lambda n: 256 * ((n + kp.RS_TILE - 1) // kp.RS_TILE)           # the histogram scan's length
    assert cells(65536) == kp.SCAN_SMALL_MAX and cells(65537) > kp.SCAN_SMALL_MAX and 65536 in kp.SORT_LENGTHS and 65537 in kp.SORT_LENGTHS


def test_rows_reference():
    for n, density in ((1, "empty"), (5, "full"), (33, "p50"), (70, "p50"), (65, "cross"), (130, "p01")):
        bits, ld = kp.bit_matrix(n, density, seed=n)
        W = ld // 64
        rows = [[int(x) for x in r] for r in bits]
        bit = lambda i, c: rows[i][c // 64] >> (c % 64) & 1
        for i in range(n):      # symmetric, zero diagonal, zero pad columns
            assert bit(i, i) == 0 and all(bit(i, c) == 0 for c in range(n, ld)) and all(bit(i, c) == bit(c, i) for c in range(n))
        ref = kp.ref_rows(bits, n, ld)
        deg = [sum(bin(w).count("1") for w in r) for r in rows]
        degp = [sum(bit(i, c) for c in range(i + 1, n)) for i in range(n)]
        cost = [sum(bit(i, c) * (W - c // 64 + 4) for c in range(i + 1, n)) for i in range(n)]
        assert ref["deg"].tolist() == deg and ref["degp"].tolist() == degp and ref["rowcost"].tolist() == cost
        assert ref["wpre"].tolist() == [[sum(bin(w).count("1") for w in r[:k]) for k in range(W)] for r in rows]
        assert ref["edge_off"].tolist() == [sum(degp[:i]) for i in range(n + 1)] and ref["total"] == sum(degp) == sum(deg) // 2
        assert ref["cost_pre"].tolist() == [sum(cost[:i]) for i in range(n + 1)]
        assert ref["ebase"].tolist() == [(sum(degp[:i]) - (deg[i] - degp[i])) % 2 ** 32 for i in range(n)]
        if density == "full":
            assert deg == [n - 1] * n
    assert 4097 in kp.ROWS_N and (4097 + 63) // 64 == 65               # W = 65: a second trip of the word loop
    assert 8192 // kp.RS_ROWS == 256                                    # 256 tiles: look-back depth 4


def test_split_reference():
    for shape in kp.SPLIT_SHAPES:
        for n in (1, 7, 64, 100):
            cost = kp.split_costs(shape, n)
            pre = [sum(cost.tolist()[:i]) for i in range(n + 1)]
            cost_pre, edge_off = np.array(pre, u64), np.arange(n + 1, dtype=u64) * u64(3)
            for world in kp.SPLIT_WORLDS:
                cuts = [0] + [next(r for r in range(n + 1) if pre[r] >= pre[n] * l // world) for l in range(1, world)] + [n]
                for rank in range(world):
                    rows, edges = kp.ref_split(cost_pre, edge_off, n, rank, world)
                    assert rows == cuts[rank:rank + 2] and edges == [3 * r for r in rows], (shape, n, world, rank)
    c = kp.split_costs("plateaus", 20000)
    assert (c == 0).sum() > 19000 and (c > 0).sum() >= 6


def test_select_reference():
    r = kp.rng(5)
    for trial in range(40):
        M = int(r.integers(1, 60))
        keys = r.integers(0, 6, M).astype(u32)          # many ties, and zeros ("no key")
        kmin = int(r.integers(1, 4))
        want = int(r.integers(1, M + 3))
        ranked = sorted((i for i in range(M) if keys[i] >= kmin), key=lambda i: (-int(keys[i]), i))
        taken = ranked[:want]
        want_eff, kstar, need_eq, sel, sel_keys = kp.ref_select(keys, kmin, want)
        assert want_eff == len(taken) and sel.tolist() == sorted(taken) and sel_keys.tolist() == [int(keys[i]) for i in sorted(taken)]
        if taken:
            assert kstar == int(keys[taken[-1]]) and need_eq == sum(int(keys[i]) == kstar for i in taken)
    store = np.arange(1, 41, dtype=u32)
    assert kp.logical_keys(store, 8, 10, [0, 3, 8]).tolist() == [0] * 8 + [11, 12, 13] + [0] * 5 + list(range(21, 29))


# ---- the case tables ----------------------------------------------------------------------------------------------------------------
def test_scan_tables():
    tiles = lambda n: (n + SCAN_TILE - 1) // SCAN_TILE
    assert kp.SCAN_SMALL_LENGTHS == [0, 1, 8191, 8192] and kp.SCAN_TILED_LENGTHS[0] == 8193
    for k in (3, 64, 65, 129):
        assert {SCAN_TILE * k - 1, SCAN_TILE * k, SCAN_TILE * k + 1} <= set(kp.SCAN_TILED_LENGTHS)
    assert max(tiles(n) for n in kp.SCAN_TILED_LENGTHS) == 130 <= kp.LB_MAX_TILES
    assert tiles(kp.SCAN_CARRY_LENGTH) > 1024
    # the all-ones totals
    assert kp.ONES_LB_N * kp.ALL_ONES == 3 * 2 ** 48 - 196608 < 2 ** 50
    assert kp.ONES_BIG_N * kp.ALL_ONES == 2 ** 52 - 2 ** 20 > 2 ** 50
    assert int(kp.ref_scan(kp.scan_values("ones", kp.ONES_LB_N))[-1]) == 3 * 2 ** 48 - 196608
    n = 5 * SCAN_TILE + 777
    rg = kp.scan_ranges(n)
    assert rg["one_tile"][0] // SCAN_TILE == (rg["one_tile"][1] - 1) // SCAN_TILE
    assert all(x % SCAN_TILE == 0 for x in rg["borders"]) and rg["empty"][0] == rg["empty"][1]
    assert rg["last_tile"][0] // SCAN_TILE == tiles(n) - 1 and rg["last_tile"][0] % SCAN_TILE and rg["last_tile"][1] <= n


def test_tie_blocks_straddle_the_borders_named():
    for name, (M, a, b, cut, n_above) in kp.TIE_BLOCKS.items():
        borders = [x for x in range(CP_TILE, M, CP_TILE) if a < x < b]      # tile borders strictly inside the block
        if name.startswith("one_border") or name.startswith("block_"):
            assert len(borders) == 1, name
        elif name.startswith("two_borders"):
            assert len(borders) == 2, name
        else:
            assert len(borders) >= 30, name
        assert a <= cut < b
        if name.endswith("cut_last_of_tile"):
            assert cut % CP_TILE == CP_TILE - 1, name
        elif name.endswith("cut_first_of_next"):
            assert cut % CP_TILE == 0, name
        elif name.endswith("cut_middle"):
            assert 16 < cut % CP_TILE < CP_TILE - 16, name
        keys, want = kp.tie_case(name)
        assert keys.min() >= 1 and keys.size == M
        assert (keys[a:b] == kp.SELECT_KSTAR).all() and (keys == kp.SELECT_KSTAR).sum() == b - a and (keys > kp.SELECT_KSTAR).sum() == n_above
        want_eff, kstar, need_eq, sel, _ = kp.ref_select(keys, int(keys.min()), want)
        assert (want_eff, kstar, need_eq) == (want, kp.SELECT_KSTAR, cut - a + 1), name
        assert max(i for i in sel.tolist() if a <= i < b) == cut, name
    assert kp.TIE_BLOCKS["block_first_entry_only"][3] == kp.TIE_BLOCKS["block_first_entry_only"][1]
    assert kp.TIE_BLOCKS["block_whole"][3] == kp.TIE_BLOCKS["block_whole"][2] - 1


def test_select_tables():
    for kind in ("random32", "one_value", "adjacent", "fp32", "fp32_floor"):
        for M in kp.SELECT_LENGTHS:
            keys, preset, kmin, kmax, rounds = kp.select_keys(kind, M, seed=M)
            assert keys.size == M and keys.min() >= 1 and keys.max() <= kmax and rounds == (2 if preset else 3), (kind, M)
            if kind == "random32" and M >= 2:
                assert kmax - kmin >= 2 ** 31                    # a window of 32 bits
            if kind.startswith("fp32"):
                assert kp.F2 <= keys.min() and keys.max() <= kp.F3 and (kmax - kmin).bit_length() <= 24     # two rounds of 12 bits
            if kind == "fp32_floor" and M >= 1023:
                assert (keys < kmin).any() and (keys >= kmin).any()      # the floor leaves keys below it
    assert {M % 4 for M in kp.SELECT_LENGTHS if M > CP_TILE} >= {1, 2, 3}
    assert {1, 3, 4, 5, 1023, 1024, 1025} <= set(kp.SELECT_LENGTHS)
    # trip ends: derived from sel_blocks by launch_select_rounds' formula
    for sel_blocks in (2, 256):
        lengths = kp.trip_end_lengths(sel_blocks)
        assert len(lengths) == 6
        for M, (trips, d) in zip(lengths, [(t, d) for t in (4, 8) for d in (-1, 0, 1)]):
            blocks = min(-(-M // (kp.SEL_THREADS * kp.SEL_ITEMS)), sel_blocks)
            assert blocks == sel_blocks == kp.select_grid(M, sel_blocks)
            assert M % 4 == 0 and M // 4 == trips * blocks * kp.SEL_THREADS + d
    assert kp.select_grid(1, 0) == 1 and kp.select_grid(10 ** 7, 0) == 256 and kp.select_grid(4097, 0) == 2
    assert -(-kp.SCANNED_M // CP_TILE) > 4096
    for segments, seg_len in kp.SEGMENT_SHAPES:
        assert seg_len % 1024 == 0
        seen = set()
        for seed in range(7):
            store, seg_stride, valid = kp.segmented_case(segments, seg_len, seed)
            seen |= set(valid)
            assert store.min() >= 1 and seg_stride % 4 == 0 and seg_stride >= seg_len
            logical = kp.logical_keys(store, seg_len, seg_stride, valid)
            assert (logical != 0).sum() == sum(valid)
            for s, nv in enumerate(valid):      # garbage behind the valid count: above every real key, so it would be selected if read
                assert (store[s * seg_stride + nv: (s + 1) * seg_stride] > kp.F3).all()
        assert seen == {0, 1, 2, 3, 5, seg_len - 1, seg_len}


def test_the_seven_match_sets_differ_per_tile():
    """Per mode, the number of matches tile 0 keeps and the prefix over tiles 0 and 1 — what the later tiles read from the descriptors —
    are different in all seven sets, and across the two modes."""
    seq = kp.epoch_sequence()
    assert len(seq) == kp.EPOCH_CALLS >= 4300 and set(seq[:, 0].tolist()) == set(range(7)) and set(seq[:, 1].tolist()) == {0, 1}
    assert (seq[1:] != seq[:-1]).any(axis=1).mean() > 0.8          # consecutive calls mostly differ
    first, both = [], []
    for m in kp.EPOCH_MODES:
        for s in range(kp.EPOCH_SETS):
            a, b = kp.epoch_set(s)
            assert a.shape == (kp.EPOCH_NS, kp.EPOCH_D) and b.shape == (kp.EPOCH_NT, kp.EPOCH_D)
            t = kp.tile_counts(match_ref.match(a, b, **m)[0])
            assert len(t) == 3 and t.min() > 0
            first.append(int(t[0])); both.append(int(t[0] + t[1]))
    assert len(set(first)) == len(first) == 14 and len(set(both)) == 14, (first, both)
