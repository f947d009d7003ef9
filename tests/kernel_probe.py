"""Kernel-level probe of the integer primitives under stage A's tail and stage B (scans, sort, row statistics, shard split, select
and compaction): the loader of tests/native/kernel_probe.hip, the numpy / Python-integer references and the case tables.

A plain module (no fixtures): the test_gpu_scan / sort / rows / shard_split / select files drive the device through it, and
test_kernel_probe_ref.py checks — without a GPU — that the probe builds, that the references agree with brute-force definitions
and that the case tables sit on the borders they are named for.  Every comparison is exact: no tolerance appears anywhere.

The probe is built with hipcc and build.py's FLAGS into tests/build/ (git-ignored) and linked against sac-cot_amd/libsaccot.so by
a relative rpath; it is rebuilt when older than its source, a header of csrc or the library (build.py's staleness rule).
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "sac-cot_amd")
SRC = os.path.join(ROOT, "tests", "native", "kernel_probe.hip")
OUT_DIR = os.path.join(ROOT, "tests", "build")
PROBE = os.path.join(OUT_DIR, "libkernel_probe.so")

# Tile sizes of the kernels under test (sc_scan.hip, sc_sort.hip, sc_rows.hip, sc_tri.hip).  The case tables below are placed by
# them; test_kernel_probe_ref.py reads each one back from the source, so a retuned kernel moves its cases or fails there.
SCAN_TILE, SCAN_SMALL_MAX = 4096, 8192
RS_TILE = 2048
RS_ROWS = 32
CP_TILE = 1024
SEL_THREADS, SEL_ITEMS = 256, 16
KP_ESCRATCH = -1001

u64, u32 = np.uint64, np.uint32

EXPORTS = {
    "kp_scan_temp_bytes": (C.c_size_t, [C.c_size_t]),
    "kp_scan": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kp_scan_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_longlong, C.c_void_p,
                               C.c_void_p]),
    "kp_sort_temp_bytes": (C.c_size_t, [C.c_size_t]),
    "kp_sort": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "kp_row_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kp_row_stats_scan_state_bytes": (C.c_size_t, [C.c_int]),
    "kp_row_stats_scan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]),
    "kp_shard_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kp_select_state_bytes": (C.c_size_t, []),
    "kp_compact_blocks": (C.c_size_t, [C.c_uint64]),
    "kp_select_scratch_bytes": (C.c_size_t, [C.c_uint64]),
    "kp_select_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]),
    "kp_select_run": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint32,
                                C.c_longlong, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kp_select_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


# ---- build and load ---------------------------------------------------------------------------------------------------------
def _build_module():
    spec = importlib.util.spec_from_file_location("saccot_build", os.path.join(PKG_DIR, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def probe_deps(b=None):
    b = b or _build_module()
    return [SRC, b.LIB] + [os.path.join(b.CSRC, h) for h in b.HEADERS]


def build_probe(force: bool = False, verbose: bool = False) -> str:
    """Compile tests/native/kernel_probe.hip when it is missing or older than what it is made from.  The library must be there."""
    b = _build_module()
    if not os.path.exists(b.LIB):
        raise RuntimeError(f"{b.LIB} is missing: build the library first (__graft_entry__.build())")
    if not force and not b._stale(PROBE, probe_deps(b)):
        return PROBE
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        raise RuntimeError(f"{PROBE} is missing or older than its sources and there is no hipcc at {hipcc} to rebuild it")
    os.makedirs(OUT_DIR, exist_ok=True)
    cmd = [hipcc] + b.FLAGS + ["-shared", SRC, "-o", PROBE, "-L" + PKG_DIR, "-lsaccot", "-Wl,-rpath,$ORIGIN/../../sac-cot_amd"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return PROBE


_lib = None


def load():
    """The probe through ctypes, built first if need be.  Raises (a failing test, never a skip) when it cannot be had."""
    global _lib
    if _lib is None:
        path = build_probe()
        # the library first, through the package: its loader lets torch bring in the process's one HIP runtime before anything else
        # does (api.load_library), and the probe's DT_NEEDED then finds libsaccot.so already there
        import sys
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.load_package().load_library()
        L = C.CDLL(path)
        for name, (res, args) in EXPORTS.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


# ---- references ---------------------------------------------------------------------------------------------------------------
def ref_scan(vals, rng_=None):
    """out (n + 1, uint64): exclusive prefix of vals, out[n] the total; rng_ = (lo, hi): the values outside [lo, hi) count as zero."""
    v = np.asarray(vals, u32).astype(u64)
    if rng_ is not None:
        i = np.arange(v.size)
        v = np.where((i >= rng_[0]) & (i < rng_[1]), v, u64(0))
    out = np.zeros(v.size + 1, u64)
    np.cumsum(v, dtype=u64, out=out[1:])
    return out


def scan_dead_tiles(n, rng_):
    """Tiles of the scan that lie wholly outside [lo, hi): neither read nor written."""
    lo, hi = rng_
    return [t for t in range((n + SCAN_TILE - 1) // SCAN_TILE) if t * SCAN_TILE + SCAN_TILE <= lo or t * SCAN_TILE >= hi]


def ref_ebase(out, deg, degp):
    """ebase[i] = (u32) out[i] - (deg[i] - degp[i]), modulo 2^32."""
    low = (np.asarray(out[:-1], u64) & u64(0xFFFFFFFF)).astype(np.int64)
    return ((low - (np.asarray(deg).astype(np.int64) - np.asarray(degp).astype(np.int64))) & 0xFFFFFFFF).astype(u32)


def ref_sort(words):
    """Stable sort by the high 32 bits (the low halves are the positions: already ascending)."""
    w = np.asarray(words, u64)
    return w[np.argsort((w >> u64(32)).astype(u32), kind="stable")]


def unpack_rows(bits, n, ld):
    """bits (n x ld/64 uint64) -> bool (n, ld): bit c of row i."""
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(n, ld // 8), axis=1, bitorder="little").astype(bool)


def ref_rows(bits, n, ld):
    """Everything the row launches owe, from popcounts of the bit matrix."""
    W = ld // 64
    A = unpack_rows(bits, n, ld)
    pc = A.reshape(n, W, 64).sum(2, dtype=np.int64)
    deg = pc.sum(1)
    wpre = np.cumsum(pc, axis=1) - pc
    A &= np.arange(ld)[None, :] > np.arange(n)[:, None]          # the bits above the diagonal
    upc = A.reshape(n, W, 64).sum(2, dtype=np.int64)
    degp = upc.sum(1)
    cost = (upc * (W - np.arange(W) + 4)[None, :]).sum(1)        # python-int sized: n * ld * (W + 4) < 2^63
    edge_off = np.concatenate([[0], np.cumsum(degp)]).astype(u64)
    cost_pre = np.concatenate([[0], np.cumsum(cost)]).astype(u64)
    return dict(deg=deg.astype(u32), degp=degp.astype(u32), wpre=wpre.astype(u32), rowcost=np.minimum(cost, 0xFFFFFFFF).astype(u32),
                cost=cost, edge_off=edge_off, cost_pre=cost_pre, ebase=ref_ebase(edge_off, deg, degp), total=int(edge_off[n]))


def ref_split(cost_pre, edge_off, n, rank, world):
    """own_row[0..1], own_edge[0..1]: boundary l is the first row whose cost prefix reaches total * l // world (Python integers)."""
    total = int(cost_pre[n])
    rows = []
    for l in (rank, rank + 1):
        if l == 0:
            rows.append(0)
        elif l >= world:
            rows.append(n)
        else:
            rows.append(int(np.searchsorted(cost_pre[:n + 1], u64(total * l // world), "left")))
    return rows, [int(edge_off[r]) for r in rows]


def ref_select(keys, kmin, want):
    """The definition.  keys: the view's logical entries (0 = no key).  Of the keys >= kmin, ordered by (key descending, ordinal
    ascending), the first want_eff = min(want, how many there are) are taken; kstar is the last key taken, need_eq how many of the
    taken equal it.  -> (want_eff, kstar, need_eq, ordinals ascending, their keys)."""
    keys = np.asarray(keys, u32)
    idx = np.flatnonzero(keys >= u32(kmin))
    k = keys[idx]
    order = np.argsort(~k, kind="stable")
    want_eff = min(int(want), idx.size)
    taken = order[:want_eff]
    if want_eff == 0:
        return 0, None, 0, np.zeros(0, u64), np.zeros(0, u32)
    kstar = int(k[taken[-1]])
    need_eq = int((k[taken] == kstar).sum())
    sel = np.sort(idx[taken])
    return want_eff, kstar, need_eq, sel.astype(u64), keys[sel]


def logical_keys(store, seg_len, seg_stride, valid):
    """A segmented view's logical entries: segment s holds valid[s] keys of store[s * seg_stride ...], the rest reads as 0."""
    out = np.zeros(len(valid) * seg_len, u32)
    for s, nv in enumerate(valid):
        out[s * seg_len: s * seg_len + nv] = store[s * seg_stride: s * seg_stride + nv]
    return out


# ---- case tables ----------------------------------------------------------------------------------------------------------------
def rng(seed):
    return np.random.default_rng(seed)


# scans: lengths around the one-block limit and around k tiles (look-back depth past one and two steps of 64)
SCAN_SMALL_LENGTHS = [0, 1, SCAN_SMALL_MAX - 1, SCAN_SMALL_MAX]
SCAN_TILED_LENGTHS = [SCAN_SMALL_MAX + 1] + [SCAN_TILE * k + d for k in (3, 64, 65, 129) for d in (-1, 0, 1) if SCAN_TILE * k + d > SCAN_SMALL_MAX]
LB_MAX_TILES, LB_MAX_TILES_RANGE = 256, 512      # launch_scan_u32: the look-back form up to here, without / with a range
SCAN_CARRY_LENGTH = SCAN_TILE * 1024 + 1234      # past 1024 tiles: a second trip of scan_of_sums_kernel's carry loop
ALL_ONES = 0xFFFFFFFF
ONES_LB_N = 196608                               # 48 tiles of 0xFFFFFFFF: 3 * 2^48 - 196 608, under the look-back's 2^50
ONES_BIG_N = 1 << 20                             # 2^52 - 2^20: past 2^50, for the forms without look-back


LB_VALUE_LIMIT = 1 << 50                         # a look-back descriptor's value field (sc_block.hpp): every prefix stays below it


def scan_values(kind, n, seed=0, lookback=False):
    """lookback: the values are bounded so that their total stays below 2^50 (the look-back form's precondition)."""
    if kind == "zero":
        return np.zeros(n, u32)
    if kind == "ones":
        assert not lookback or n * ALL_ONES < LB_VALUE_LIMIT
        return np.full(n, ALL_ONES, u32)
    top = min(1 << 32, (LB_VALUE_LIMIT - 1) // max(n, 1) + 1) if lookback else 1 << 32
    return rng(seed).integers(0, top, n, dtype=u64).astype(u32)


def scan_ranges(n):
    """[lo, hi) cases for a length of at least four tiles: inside one tile, on tile borders, empty, inside the last partial tile."""
    last0 = (n - 1) // SCAN_TILE * SCAN_TILE
    return {"one_tile": (SCAN_TILE + 100, SCAN_TILE + 1500), "borders": (SCAN_TILE, 3 * SCAN_TILE), "empty": (2 * SCAN_TILE, 2 * SCAN_TILE),
            "empty_front": (0, 0), "last_tile": (last0 + (n - last0) // 4, n - 1 if n - last0 > 2 else n), "all": (0, n)}


SORT_LENGTHS = [1, 63, 64, 65, RS_TILE - 1, RS_TILE, RS_TILE + 1, 65536, 65537, 1000003]
SORT_PATTERNS = ["random", "equal", "two", "descending", "top_byte", "low_byte"]


def sort_words(pattern, n, seed=0):
    r = rng(seed)
    if pattern == "random":
        hi = r.integers(0, 1 << 32, n, dtype=u64)
    elif pattern == "equal":
        hi = np.full(n, 0x89ABCDEF, u64)
    elif pattern == "two":
        hi = np.where(r.integers(0, 2, n) == 1, u64(0xFFFF0000), u64(0x0000FFFF))
    elif pattern == "descending":
        hi = (u64(0xFFFFFFFF) - np.arange(n, dtype=u64) // u64(3))
    elif pattern == "top_byte":      # bits 56 .. 63 of the word
        hi = r.integers(0, 256, n, dtype=u64) << u64(24) | u64(0x00123456)
    elif pattern == "low_byte":      # bits 32 .. 39
        hi = r.integers(0, 256, n, dtype=u64) | u64(0xABCDEF00)
    else:
        raise ValueError(pattern)
    return (hi << u64(32)) | np.arange(n, dtype=u64)


ROWS_N = [1, 31, 32, 33, 63, 64, 65, 2049, 4097, 8192]
ROWS_DENSITIES = ["empty", "full", "p01", "p50", "cross"]


def bit_matrix(n, density, seed=0):
    """A symmetric bit matrix with zero diagonal and zero pad columns: (n x ld/64 uint64, ld)."""
    ld = (n + 63) // 64 * 64
    A = np.zeros((n, ld), bool)
    if density == "full":
        A[:, :n] = True
    elif density in ("p01", "p50"):
        up = np.triu(rng(seed).random((n, n), dtype=np.float32) < (0.01 if density == "p01" else 0.5), 1)
        A[:, :n] = up | up.T
    elif density == "cross":
        A[n // 2, :n] = True
        A[:n, n // 2] = True
    elif density != "empty":
        raise ValueError(density)
    A[np.arange(n), np.arange(n)] = False
    return np.packbits(A, axis=1, bitorder="little").view(u64).reshape(n, ld // 64).copy(), ld


SPLIT_N = [1, 63, 64, 65, 4097, 20000]
SPLIT_WORLDS = [1, 2, 3, 8, 64]
SPLIT_SHAPES = ["uniform", "zero", "heavy_start", "heavy_middle", "heavy_end", "plateaus", "increasing"]


def split_costs(shape, n, seed=0):
    """Per-row costs (uint64, n) of a shard-split case."""
    c = np.zeros(n, u64)
    if shape == "uniform":
        c[:] = 7
    elif shape == "heavy_start":
        c[:] = 1; c[0] = 10 * n + 5
    elif shape == "heavy_middle":
        c[:] = 1; c[n // 2] = 10 * n + 5
    elif shape == "heavy_end":
        c[:] = 1; c[n - 1] = 10 * n + 5
    elif shape == "plateaus":     # a few equal spikes, zero rows between them: boundaries of every world land on or next to a plateau
        c[:: max(1, n // 6)] = 1000
    elif shape == "increasing":
        c[:] = np.arange(1, n + 1, dtype=u64) * u64(3)
    elif shape != "zero":
        raise ValueError(shape)
    return c


# ---- select --------------------------------------------------------------------------------------------------------------------
F2, F3 = 0x40000000, 0x40400000     # the bit patterns of 2.0f and 3.0f: the key kernel's preset window


def select_grid(M, sel_blocks):
    """Workgroups of a select round: launch_select_rounds' rule."""
    blocks = (M + SEL_THREADS * SEL_ITEMS - 1) // (SEL_THREADS * SEL_ITEMS)
    cap = sel_blocks if sel_blocks >= 1 else 256
    return max(1, min(blocks, cap))


def trip_end_lengths(sel_blocks):
    """M with M / 4 one below, on and above 4 and 8 grid strides: the ends of select_round_kernel's four-deep loop and of its
    remainder loop, for a grid of sel_blocks workgroups (each length really gets that grid)."""
    stride = sel_blocks * SEL_THREADS
    out = []
    for trips in (4, 8):
        for d in (-1, 0, 1):
            M = 4 * (trips * stride + d)
            assert select_grid(M, sel_blocks) == sel_blocks, (M, sel_blocks)
            out.append(M)
    return out


def select_keys(kind, M, seed=0):
    """Key arrays (all >= 1) -> (keys, preset, kmin, kmax, rounds).  preset 0: the measured range in three rounds; 1: the preset
    window [floor, 3.0] in two."""
    r = rng(seed)
    if kind == "random32":
        k = r.integers(1, 1 << 32, M, dtype=u64).astype(u32)
        if M >= 2:
            k[r.choice(M, 2, replace=False)] = [1, 0xFFFFFFFF]            # the window really spans 32 bits
    elif kind == "one_value":
        k = np.full(M, 0x12345678, u32)
    elif kind == "adjacent":
        k = (u32(0x40000000) + r.integers(0, 2, M).astype(u32)).astype(u32)
    elif kind in ("fp32", "fp32_floor"):
        k = r.uniform(2.0, 3.0, M).astype(np.float32).view(u32).copy()
        k[r.integers(0, M, max(1, M // 50))] = F3           # some keys at the top of the window
        if M >= 8:
            k[r.integers(0, M, M // 8)] = k[0]               # ... and ties
        floor = F2 if kind == "fp32" else int(np.float32(2.6).view(u32))
        return k, 1, floor, F3, 2
    else:
        raise ValueError(kind)
    return k, 0, int(k.min()), int(k.max()), 3


SELECT_LENGTHS = [1, 3, 4, 5, 1023, 1024, 1025, 3 * CP_TILE + 1, 3 * CP_TILE + 2, 5 * CP_TILE + 3]
SCANNED_M = 4096 * CP_TILE + 1025          # past compact_self_max's 4096 tiles: the compaction with the scan launch
SELECT_KSTAR = 0x40200000

# name -> (M, [a, b): the block of keys == k*, position of the LAST key taken, keys above k*).  The cut is named by where that
# position sits in its tile of CP_TILE entries; the block by how many tile borders lie strictly inside it.
TIE_BLOCKS = {
    "one_border_cut_last_of_tile": (4 * CP_TILE, 1000, 1100, CP_TILE - 1, 7),
    "one_border_cut_first_of_next": (4 * CP_TILE, 1000, 1100, CP_TILE, 7),
    "one_border_cut_middle": (4 * CP_TILE, 1000, 1100, 1050, 0),
    "two_borders_cut_last_of_tile": (5 * CP_TILE + 3, 900, 2100, 2 * CP_TILE - 1, 33),
    "two_borders_cut_first_of_next": (5 * CP_TILE + 3, 900, 2100, 2 * CP_TILE, 33),
    "two_borders_cut_middle": (5 * CP_TILE + 3, 900, 2100, 1500, 33),
    "many_borders_cut_last_of_tile": (40 * CP_TILE + 1, 500, 37 * CP_TILE + 5, 20 * CP_TILE - 1, 1000),
    "many_borders_cut_first_of_next": (40 * CP_TILE + 1, 500, 37 * CP_TILE + 5, 20 * CP_TILE, 1000),
    "many_borders_cut_middle": (40 * CP_TILE + 1, 500, 37 * CP_TILE + 5, 20 * CP_TILE + 511, 1000),
    "block_first_entry_only": (4 * CP_TILE, 1000, 1100, 1000, 7),        # need_eq == 1
    "block_whole": (4 * CP_TILE, 1000, 1100, 1099, 7),                   # need_eq == the whole block
}


def tie_case(name, seed=0):
    """-> (keys, want): keys == SELECT_KSTAR on [a, b), n_above keys above it elsewhere, the rest below; want = the keys above plus the
    block's entries up to and including the cut position."""
    M, a, b, cut, n_above = TIE_BLOCKS[name]
    r = rng(seed)
    k = r.integers(1, SELECT_KSTAR, M, dtype=u64).astype(u32)
    outside = np.concatenate([np.arange(0, a), np.arange(b, M)])
    k[r.choice(outside, n_above, replace=False)] = r.integers(SELECT_KSTAR + 1, 1 << 32, n_above, dtype=u64).astype(u32)
    k[a:b] = SELECT_KSTAR
    return k, n_above + (cut - a + 1)


SEGMENT_SHAPES = [(2, 1024), (3, 1024), (8, 1024), (2, 4096), (3, 4096), (8, 4096)]


def segment_valids(seg_len):
    return [0, 1, 2, 3, 5, seg_len - 1, seg_len]


def segmented_case(segments, seg_len, seed=0):
    """-> (store, seg_stride, valid): garbage (never 0, so it would count if it were read) behind every segment's valid count; the
    valid counts walk through segment_valids, rotated by the seed."""
    r = rng(seed)
    seg_stride = seg_len + 64                         # room between the segments, as a blob's header and records leave
    store = r.integers(0x41000000, 1 << 32, segments * seg_stride, dtype=u64).astype(u32)   # garbage: above every real key
    vs = segment_valids(seg_len)
    valid = [vs[(seed + s) % len(vs)] for s in range(segments)]
    for s, nv in enumerate(valid):
        real = r.uniform(2.0, 3.0, nv).astype(np.float32).view(u32)
        if nv >= 4:
            real[r.integers(0, nv, nv // 4)] = real[0]    # ties
        store[s * seg_stride: s * seg_stride + nv] = real
    return store, seg_stride, valid


# ---- look-back epochs through the public API (tests/test_gpu_lookback_epochs.py) -----------------------------------------------
EPOCH_NS, EPOCH_NT, EPOCH_D, EPOCH_SETS, EPOCH_CALLS = 700, 64, 3, 7, 4400
EPOCH_MODES = [dict(knn=1, mutual=True), dict(knn=1, ratio=0.8)]
FIN_TILE = 256                                        # source rows per tile of the match's finishing launch (sc_match.hip)


def epoch_set(s):
    """Descriptor set s: every target row is an exact copy of a source row of its own, 4 + 2 s of them from the first tile of 256
    source rows and 10 + 3 s from the second — so in mutual mode the tiles keep a different number of matches in every set (in ratio
    mode the seeds see to it: test_kernel_probe_ref.py asserts both)."""
    r = rng(9200 + s)
    a = r.standard_normal((EPOCH_NS, EPOCH_D)).astype(np.float32)
    c0, c1 = 4 + 2 * s, 10 + 3 * s
    rows = np.concatenate([r.choice(FIN_TILE, c0, replace=False), FIN_TILE + r.choice(FIN_TILE, c1, replace=False),
                           2 * FIN_TILE + r.choice(EPOCH_NS - 2 * FIN_TILE, EPOCH_NT - c0 - c1, replace=False)])
    return a, a[r.permutation(rows)].copy()


def epoch_sequence():
    """Which (set, mode) call k uses: a fixed seeded sequence."""
    r = rng(4242)
    return np.stack([r.integers(0, EPOCH_SETS, EPOCH_CALLS), r.integers(0, len(EPOCH_MODES), EPOCH_CALLS)], axis=1)


def tile_counts(corr):
    """Matches kept per finishing tile, from a reference's correspondence list."""
    return np.bincount(np.asarray(corr)[:, 0] // FIN_TILE, minlength=(EPOCH_NS + FIN_TILE - 1) // FIN_TILE)


# ---- device runners (GPU tests only: torch is imported here, not at module level) -----------------------------------------------
GUARD = 4096
SENT = 0xA5
SENT32, SENT64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


class DevBuf:
    """nbytes of device memory straight from the allocator, with GUARD bytes behind it; everything starts as the sentinel byte,
    then `data` (a numpy array) or zeros where asked."""

    def __init__(self, nbytes, data=None, zero=False):
        import torch
        self.nbytes = int(nbytes)
        self.t = torch.full((self.nbytes + GUARD,), SENT, dtype=torch.uint8, device="cuda")
        if zero:
            self.t[:self.nbytes] = 0
        if data is not None:
            raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert raw.size <= self.nbytes
            if raw.size:
                self.t[:raw.size] = torch.from_numpy(raw.copy()).cuda()

    @classmethod
    def of(cls, data):
        return cls(np.asarray(data).nbytes, data)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def read(self, dtype):
        return self.t[:self.nbytes].cpu().numpy().view(dtype)

    def guard_ok(self):
        return bool((self.t[self.nbytes:] == SENT).all().item())


class Pinned:
    """One u64 of host-pinned memory, preset to a sentinel."""

    def __init__(self, value=SENT64):
        import torch
        self.t = torch.zeros(1, dtype=torch.int64).pin_memory()
        self.t.numpy().view(u64)[0] = value

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        return int(self.t.numpy().view(u64)[0])


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch
    torch.cuda.synchronize()


class LbState:
    """A look-back state area as lb_next keeps it: ticket and error words in a buffer of their own (zeroed once), the descriptor
    area zeroed when new and when the caller says so (the epoch's wrap)."""

    def __init__(self, desc_bytes):
        self.words = DevBuf(64, zero=True)         # ticket at +0, err at +32
        self.desc = DevBuf(desc_bytes, zero=True)

    def zero_desc(self):
        self.desc.t[:self.desc.nbytes] = 0

    @property
    def ticket(self):
        return self.words.ptr

    @property
    def err(self):
        return self.words.ptr + 32

    def clean(self):
        """ticket back at zero, no error reported, nothing written behind either buffer"""
        w = self.words.read(u32)
        return int(w[0]) == 0 and int(w[8]) == 0 and self.words.guard_ok() and self.desc.guard_ok()


def run_scan(vals, form, *, rng_=None, lb=None, epoch=0, with_ebase=False, with_host=False, seed=0):
    """One launch_scan_u32.  form: "lookback" (lb, epoch given), "self" (no LbArgs), "three" (scan_self_max = 0); a length up to
    SCAN_SMALL_MAX takes the one-block kernel whatever the form.  -> dict(out (n + 1 words, untouched ones still the sentinel),
    ebase, host, ok (every guard intact, look-back words clean))."""
    L = load()
    vals = np.asarray(vals, u32)
    n = vals.size
    d_in = DevBuf.of(vals)
    d_out = DevBuf((n + 1) * 8)
    tb = L.kp_scan_temp_bytes(n)
    d_tmp = DevBuf(tb)
    d_rng = DevBuf.of(np.asarray(rng_, u64)) if rng_ is not None else None
    deg = degp = d_deg = d_degp = d_eb = None
    if with_ebase:
        r = rng(seed + 77)
        degp = r.integers(0, 1 << 20, n, dtype=u64).astype(u32)
        deg = (degp + r.integers(0, 1 << 20, n, dtype=u64).astype(u32)).astype(u32)
        d_deg, d_degp, d_eb = DevBuf.of(deg), DevBuf.of(degp), DevBuf(n * 4)
    host = Pinned() if with_host else None
    use_lb = form == "lookback"
    rc = L.kp_scan(d_in.ptr, n, d_out.ptr, d_tmp.ptr, tb, 0 if form == "three" else -1, lb.ticket if use_lb else None,
                   lb.err if use_lb else None, lb.desc.ptr if use_lb else None, epoch if use_lb else 0, d_rng.ptr if d_rng else None,
                   d_deg.ptr if with_ebase else None, d_degp.ptr if with_ebase else None, d_eb.ptr if with_ebase else None,
                   host.ptr if host else None, stream())
    assert rc == 0, rc
    sync()
    ok = d_in.guard_ok() and d_out.guard_ok() and d_tmp.guard_ok() and (not with_ebase or d_eb.guard_ok()) and (not use_lb or lb.clean())
    return dict(out=d_out.read(u64), ebase=d_eb.read(u32) if with_ebase else None, deg=deg, degp=degp, host=host.get() if host else None,
                ok=ok, input_kept=np.array_equal(d_in.read(u32), vals))


def expect_scan(vals, rng_=None):
    """What run_scan's `out` must be, word for word: the prefix, with the sentinel in every tile wholly outside the range (the
    one-block form knows no range)."""
    n = len(vals)
    exp = ref_scan(vals, rng_)
    if rng_ is not None and n > SCAN_SMALL_MAX:
        for t in scan_dead_tiles(n, rng_):
            exp[t * SCAN_TILE: min(n, (t + 1) * SCAN_TILE)] = u64(SENT64)
    return exp


def run_select(keys_buf, M, *, kmin, kmax, preset, want, rounds, want_req=0, sel_blocks=0, compact_self_max=-1, seg=None, state=None,
               fresh=True):
    """kp_select_init + kp_select_run + kp_select_read on a key array already on the device.  seg = (seg_len, seg_stride, valid
    DevBuf).  -> dict(kstar, done, want, need_eq, hist (3 x 4096), ord, key (n_sel entries each, untouched ones the sentinel), short,
    self_summed, ok, state)."""
    L = load()
    state = state or DevBuf(L.kp_select_state_bytes())
    n_sel = max(1, min(int(want), int(M)))
    d_ord, d_key = DevBuf(n_sel * 8), DevBuf(n_sel * 4)
    sb = L.kp_select_scratch_bytes(M)
    d_scr = DevBuf(sb)
    short = Pinned(0)
    self_summed = C.c_int(-1)
    st = stream()
    rc = L.kp_select_init(state.ptr, 1 if fresh else 0, preset, kmin, kmax, want, want_req, st)
    assert rc == 0, rc
    seg_len, seg_stride, d_valid = seg if seg else (0, 0, None)
    rc = L.kp_select_run(keys_buf.ptr, M, seg_len, seg_stride, d_valid.ptr if d_valid else None, 1, state.ptr, rounds, sel_blocks,
                         compact_self_max, d_scr.ptr, sb, d_ord.ptr, d_key.ptr, n_sel, short.ptr, C.byref(self_summed), st)
    assert rc == 0, rc
    res = np.zeros(4, u64)
    hist = np.zeros((3, 4096), u32)
    rc = L.kp_select_read(state.ptr, res.ctypes.data, hist.ctypes.data, st)
    assert rc == 0, rc
    sync()
    ok = keys_buf.guard_ok() and d_ord.guard_ok() and d_key.guard_ok() and d_scr.guard_ok() and state.guard_ok()
    return dict(kstar=int(res[0]), done=int(res[1]), want=int(res[2]), need_eq=int(res[3]), hist=hist, ord=d_ord.read(u64), key=d_key.read(u32),
                short=short.get(), self_summed=self_summed.value, ok=ok, state=state)


def check_select(got, keys_logical, kmin, want, tag=""):
    """A select's result against the definition, every word: the state, the selection, and the sentinel behind its count."""
    want_eff, kstar, need_eq, sel, sel_keys = ref_select(keys_logical, kmin, want)
    print(tag, "want_eff", want_eff, "kstar", kstar, "need_eq", need_eq, "| got", got["want"], got["kstar"], got["need_eq"], "done", got["done"])
    assert got["ok"], (tag, "a guard behind a buffer was written")
    assert got["done"] == 1 and got["want"] == want_eff and got["need_eq"] == need_eq, tag
    if want_eff:
        assert got["kstar"] == kstar, tag
    assert np.array_equal(got["ord"][:want_eff], sel), tag
    assert np.array_equal(got["key"][:want_eff], sel_keys), tag
    assert (got["ord"][want_eff:] == u64(SENT64)).all() and (got["key"][want_eff:] == u32(SENT32)).all(), (tag, "written behind the count")
    assert not got["hist"].any(), (tag, "the histograms are not zero behind the select")
    return want_eff


def select_twice(keys_buf, M, keys_logical, tag="", **kw):
    """A select on a fresh state, then the same select on the state it left (histograms as the first left them): both equal the
    definition."""
    a = run_select(keys_buf, M, **kw)
    n = check_select(a, keys_logical, kw["kmin"], kw["want"], tag)
    b = run_select(keys_buf, M, state=a["state"], fresh=False, **kw)
    check_select(b, keys_logical, kw["kmin"], kw["want"], tag + " (again)")
    return a, n
