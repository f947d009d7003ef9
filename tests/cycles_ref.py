"""CPU restatement of sc_pairs_cycles (include/saccot.h): the reference the GPU tests compare against bit for bit, and the input
families they share.

The arithmetic is numpy float64 on the exactly widened float32 entries, every product and every sum written out element by element in
the header's order — no `@`, no dot, no einsum: a BLAS may fuse or reorder.  (A numpy ufunc call rounds once per operation.)  The
thresholds are arguments: the GPU tests pass the two values sc_cycles_thresholds returns.  The families are built with whatever is
convenient; only `cycles` is the reference.  The families of tests/test_gpu_pairs_cycles_range.py stand at the end, with what the reference
measures on them as literals; exact24 brings an integer evaluation of its own, which shares no code with `cycles`.
"""
import functools
import itertools

import numpy as np

SC_OK, SC_EINVAL = 0, -1
STATUS = 1  # SC_CYCLES_STATUS
RESULT_DTYPE = np.dtype({"names": ["status", "cycles", "ok", "ok_alive", "alive", "dropped_round", "min_trace", "max_e2", "reserved"],
                         "formats": ["<i4", "<u4", "<u4", "<u4", "<u4", "<u4", "<f8", "<f8", ("<u4", (2,))],
                         "offsets": [0, 4, 8, 12, 16, 20, 24, 32, 40], "itemsize": 48})
SUMMARY_DTYPE = np.dtype({"names": ["rounds", "stable", "alive", "edges", "triangles", "consistent"],
                          "formats": ["<u4", "<u4", "<u4", "<u4", "<u8", "<u8"], "offsets": [0, 4, 8, 12, 16, 24], "itemsize": 32})


# ---- the arithmetic: a transform is (R, t), R[i][j] and t[i] arrays over whatever is computed at once -------------------------------
def _widen(rt):
    rt = np.asarray(rt, np.float32).reshape(-1, 12).astype(np.float64)  # exact
    return [[rt[:, 3 * i + j] for j in range(3)] for i in range(3)], [rt[:, 9 + i] for i in range(3)]


def _inverse(R, t):
    """(R^T, t'), t'_c = -((R_0c t_0 + R_1c t_1) + R_2c t_2)"""
    return [[R[j][i] for j in range(3)] for i in range(3)], [-((R[0][c] * t[0] + R[1][c] * t[1]) + R[2][c] * t[2]) for c in range(3)]


def _compose(B, A):
    """M = B o A"""
    (BR, Bt), (AR, At) = B, A
    MR = [[((BR[i][0] * AR[0][j] + BR[i][1] * AR[1][j]) + BR[i][2] * AR[2][j]) for j in range(3)] for i in range(3)]
    Mt = [((BR[i][0] * At[0] + BR[i][1] * At[1]) + BR[i][2] * At[2]) + Bt[i] for i in range(3)]
    return MR, Mt


def _take(T, idx):
    return [[T[0][i][j][idx] for j in range(3)] for i in range(3)], [T[1][i][idx] for i in range(3)]


def _where(c, X, Y):
    return [[np.where(c, X[0][i][j], Y[0][i][j]) for j in range(3)] for i in range(3)], [np.where(c, X[1][i], Y[1][i]) for i in range(3)]


def _order_key(x):
    """a double as a uint64 whose order is the numbers' order, -0 below +0 (the extrema are taken in this total order)"""
    b = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def _order_value(k):
    k = np.asarray(k, np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & np.uint64((1 << 63) - 1), ~k).astype(np.uint64).view(np.float64)


def triangles(pairs, edge):
    """every triangle of the pairs that are edges: (p, q, r) index arrays, p on {a, b}, q on {b, c}, r on {a, c}, a < b < c"""
    on = {}
    for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        if edge[p]:
            on.setdefault((min(a, b), max(a, b)), []).append(p)
    above = {}
    for a, b in on:
        above.setdefault(a, set()).add(b)
    out = []
    for (a, b), ps in on.items():
        for c in sorted(above.get(a, set()) & above.get(b, set())):  # c > b > a
            out.extend(itertools.product(ps, on[(b, c)], on[(a, c)]))
    tri = np.array(out, np.int64).reshape(-1, 3)
    return tri[:, 0], tri[:, 1], tri[:, 2]


def errors(pairs, rt, tp, tq, tr_):
    """(tr, e2) of the triangles: E = T_r(c -> a) o (T_q(b -> c) o T_p(a -> b))"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    stored = _widen(rt)
    inv = _inverse(*stored)
    fwd = pairs[:, 0] < pairs[:, 1]  # stored (lower, higher)
    up, down = _where(fwd, stored, inv), _where(fwd, inv, stored)  # lower -> higher, higher -> lower
    with np.errstate(all="ignore"):
        E = _compose(_take(down, tr_), _compose(_take(up, tq), _take(up, tp)))
        tr = (E[0][0][0] + E[0][1][1]) + E[0][2][2]
        e2 = (E[1][0] * E[1][0] + E[1][1] * E[1][1]) + E[1][2] * E[1][2]
    return tr, e2


def cycles(n_sets, pairs, rt, tr_min, e2_max, min_ok=1, max_rounds=16, keep=None, statuses=None):
    """-> (records (P,) of RESULT_DTYPE, summary: one record of SUMMARY_DTYPE).  statuses: the int32 at byte 48 of every record
    (SC_CYCLES_STATUS), or None."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P = len(pairs)
    assert pairs.max() < n_sets
    rt = np.asarray(rt, np.float32).reshape(P, 12)
    status = np.zeros(P, np.int32) if statuses is None else np.asarray(statuses, np.int32).copy()
    status[(status == SC_OK) & ~np.isfinite(rt).all(axis=1)] = SC_EINVAL
    edge = (status == SC_OK) & (pairs[:, 0] != pairs[:, 1])
    keep = np.zeros(P, bool) if keep is None else np.asarray(keep).reshape(P) != 0
    tp, tq, tr_ = triangles(pairs, edge)
    safe = np.where(edge[:, None], rt, 0).astype(np.float32)  # (what is no edge is in no triangle)
    tr, e2 = errors(pairs, safe, tp, tq, tr_)
    good = (tr >= tr_min) & (e2 <= e2_max)
    res = np.zeros(P, RESULT_DTYPE)
    res["status"] = status
    kmin = np.full(P, np.uint64(2**64 - 1)); kmax = np.full(P, _order_key(np.zeros(1))[0])
    for role in (tp, tq, tr_):
        res["cycles"] += np.bincount(role, minlength=P).astype(np.uint32)
        res["ok"] += np.bincount(role[good], minlength=P).astype(np.uint32)
        np.minimum.at(kmin, role, _order_key(tr))
        np.maximum.at(kmax, role, _order_key(e2))
    res["min_trace"] = np.where(res["cycles"] > 0, _order_value(kmin), 3.0)
    res["max_e2"] = _order_value(kmax)
    alive = edge.copy()
    K, stable = max_rounds, 0
    for k in range(1, max_rounds + 1):
        live = good & alive[tp] & alive[tq] & alive[tr_]
        ok_k = sum(np.bincount(role[live], minlength=P) for role in (tp, tq, tr_))
        res["ok_alive"] = np.where(alive, ok_k, 0)
        nxt = alive & ((ok_k >= min_ok) | keep)
        res["dropped_round"][alive & ~nxt] = k
        same = bool((nxt == alive).all())
        alive = nxt
        if same:
            K, stable = k, 1
            break
    res["alive"] = alive
    summary = np.zeros(1, SUMMARY_DTYPE)
    summary["rounds"], summary["stable"], summary["alive"], summary["edges"] = K, stable, alive.sum(), edge.sum()
    summary["triangles"], summary["consistent"] = len(tp), good.sum()
    return res, summary[0]


# ---- the input families ---------------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def absolute_poses(n_sets, seed):
    """a random placement of every set in one world: x_world = R_s x + t_s"""
    rng = np.random.default_rng(seed)
    return [rotation(rng.normal(size=3), rng.uniform(0, np.pi)) for _ in range(n_sets)], rng.uniform(-1, 1, (n_sets, 3))


def relative_poses(pairs, R, t):
    """pair (a, b): the float32 Rt[12] that maps set a's coordinates onto set b's, from the absolute poses, rounded once"""
    out = np.zeros((len(pairs), 12), np.float32)
    for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        out[p, :9] = (R[b].T @ R[a]).ravel()
        out[p, 9:] = R[b].T @ (t[a] - t[b])
    return out


def corrupt(rt, which, seed, lo_deg=5.0, hi_deg=90.0):
    """the listed poses turned by lo_deg .. hi_deg about a random axis: a wrong registration that is still a rigid motion"""
    rng = np.random.default_rng(seed)
    rt = rt.copy()
    for p in which:
        W = rotation(rng.normal(size=3), np.deg2rad(rng.uniform(lo_deg, hi_deg)))
        rt[p, :9] = (W @ rt[p, :9].astype(np.float64).reshape(3, 3)).ravel()
    return rt


class Family:
    def __init__(self, n_sets, pairs, rt, bad=(), keep=None, **params):
        self.n_sets, self.pairs, self.rt = n_sets, np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2), np.ascontiguousarray(rt, np.float32)
        self.bad = np.array(sorted(bad), np.int64)
        self.keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        self.params = params  # rot_tol, trans_tol, min_ok, max_rounds as the family is used


K24_SEED, K24_BAD = 2014, 28  # (the seed at which the 28 corrupted pairs break 548 of the 2024 triangles)
ROT_TOL, TRANS_TOL = float(np.deg2rad(0.5)), 0.01


@functools.lru_cache(maxsize=None)
def k24():
    """24 sets, all 276 pairs in random stored directions and shuffled order; 28 pairs corrupted by 5 - 90 degrees"""
    rng = np.random.default_rng(K24_SEED)
    pairs = np.array(list(itertools.combinations(range(24), 2)))
    flip = rng.random(len(pairs)) < 0.5
    pairs[flip] = pairs[flip][:, ::-1]
    pairs = pairs[rng.permutation(len(pairs))]
    R, t = absolute_poses(24, K24_SEED + 1)
    bad = rng.choice(len(pairs), K24_BAD, replace=False)
    return Family(24, pairs, corrupt(relative_poses(pairs, R, t), bad, K24_SEED + 2), bad, rot_tol=ROT_TOL, trans_tol=TRANS_TOL)


@functools.lru_cache(maxsize=None)
def k24_repeats():
    """k24 with four pairs listed twice (the copies' poses clean) and three of them also listed reversed (the inverse pose, rounded)"""
    f = k24()
    clean = [p for p in range(len(f.pairs)) if p not in set(f.bad.tolist())][:4]
    R, t = absolute_poses(24, K24_SEED + 1)
    twice, back = f.pairs[clean], f.pairs[clean[:3]][:, ::-1]
    pairs = np.concatenate([f.pairs, twice, back])
    rt = np.concatenate([f.rt, relative_poses(twice, R, t), relative_poses(back, R, t)])
    return Family(24, pairs, rt, f.bad, rot_tol=ROT_TOL, trans_tol=TRANS_TOL)


@functools.lru_cache(maxsize=None)
def strip(n=42):
    """n sets in a row: chain pairs (i, i + 1), protected pairs (i, i + 2), the last chain pair protected too; min_ok 2 unravels the
    chain from its first pair, one pair a round"""
    chain = [(i, i + 1) for i in range(n - 1)]
    skip = [(i, i + 2) for i in range(n - 2)]
    pairs = np.array(chain + skip)
    keep = np.array([0] * (n - 2) + [1] + [1] * len(skip), np.uint8)
    R, t = absolute_poses(n, 7)
    return Family(n, pairs, relative_poses(pairs, R, t), keep=keep, rot_tol=ROT_TOL, trans_tol=TRANS_TOL, min_ok=2)


@functools.lru_cache(maxsize=None)
def hub(n=1500):
    """set 0 paired with every other set, ring pairs (i, i + 1) among the others: set 0's neighbour list is longer than a workgroup;
    every 50th ring pair is corrupted"""
    spokes = [(0, i) if i % 3 else (i, 0) for i in range(1, n)]
    ring = [(i, i + 1) for i in range(1, n - 1)]
    pairs = np.array(spokes + ring)
    R, t = absolute_poses(n, 11)
    bad = [len(spokes) + j for j in range(0, len(ring), 50)]
    return Family(n, pairs, corrupt(relative_poses(pairs, R, t), bad, 12), bad, rot_tol=ROT_TOL, trans_tol=TRANS_TOL)


def one_triangle(directions, consistent):
    """sets 0, 1, 2 and their three pairs, pair k stored reversed where bit k of `directions` is set; not consistent: the third pose
    is turned by 30 degrees"""
    R, t = absolute_poses(3, 5)
    pairs = np.array([(0, 1), (1, 2), (0, 2)])
    for k in range(3):
        if directions >> k & 1:
            pairs[k] = pairs[k][::-1]
    rt = relative_poses(pairs, R, t)
    if not consistent:
        rt = corrupt(rt, [2], 6, 30.0, 30.0)
    return Family(3, pairs, rt, () if consistent else (2,), rot_tol=ROT_TOL, trans_tol=TRANS_TOL)


# ---- the families of the range tests: past one trip of either loop, on the cuts, at the ends of the number range ---------------------
# k130: what the reference measures, asserted by tests/test_cycles_abi.py.  Without keep, min_ok <= 103 stops after 2 rounds with only the
# corrupted pairs gone and min_ok 104 .. 111 unravels the whole list; with every pair among the first 40 sets kept, min_ok 104 leaves
# those 780 pairs after 12 rounds, and the 193 pairs of the second grid trip (index >= 8192) leave in nine different rounds
# ([14 alive, 7, 0, 2, 2, 3, 0, 3, 8, 31, 108, 15]).
K130_SEED, K130_BAD = 130, 419  # (5 % of the 8385 pairs corrupted)
K130_PROTECTED, K130_MIN_OK = 40, 104  # every pair among the sets below K130_PROTECTED is kept
K130_SUMMARY = (12, 1, 780, 8385, 357760, 306786)  # rounds, stable, alive, edges, triangles, consistent
K130_DROPS = [780, 379, 5, 36, 133, 242, 25, 131, 406, 1182, 4344, 722, 0]  # pairs by dropped_round: [alive, round 1, ..., round 12]
K130_SHORT = 5  # a max_rounds below K130_SUMMARY's: stable == 0
K130_NO_KEEP = (12, 1, 0)  # rounds, stable, alive with keep NULL ([0, 420, 5, 40, 199, 207, 29, 162, 481, 1723, 4748, 371] by round)
# the repeats' copies close loops of their own: min_ok 104 .. 108 stops after 2 rounds, 110 unravels to the kept pairs in 9
# ([795, 389, 113, 121, 222, 348, 1290, 4332, 975] by round)
K130_REPEATS_MIN_OK, K130_REPEATS_SUMMARY = 110, (9, 1, 795, 8585, 383994, 330422)


def _complete(n, rng):
    """every pair of n sets, in random stored directions and shuffled order"""
    pairs = np.array(list(itertools.combinations(range(n), 2)))
    flip = rng.random(len(pairs)) < 0.5
    pairs[flip] = pairs[flip][:, ::-1]
    return pairs[rng.permutation(len(pairs))]


@functools.lru_cache(maxsize=None)
def k130():
    """130 sets, all 8385 pairs in random stored directions and shuffled order, 419 corrupted: more pairs than a round's grid has
    waves (2048 x 4), and every neighbour list has 129 entries — three trips of a wave's lanes"""
    rng = np.random.default_rng(K130_SEED)
    pairs = _complete(130, rng)
    R, t = absolute_poses(130, K130_SEED + 1)
    bad = rng.choice(len(pairs), K130_BAD, replace=False)
    keep = (pairs.max(axis=1) < K130_PROTECTED).astype(np.uint8)
    return Family(130, pairs, corrupt(relative_poses(pairs, R, t), bad, K130_SEED + 2), bad, keep=keep, rot_tol=ROT_TOL, trans_tol=TRANS_TOL,
                  min_ok=K130_MIN_OK, max_rounds=64)


@functools.lru_cache(maxsize=None)
def k130_repeats():
    """k130 with 200 of its pairs listed a second time (the copies' poses clean), 100 of those reversed: runs of equal neighbours
    inside lists that are longer than a wave"""
    f = k130()
    which = np.random.default_rng(K130_SEED + 3).choice(len(f.pairs), 200, replace=False)
    again = f.pairs[which].copy()
    again[:100] = again[:100, ::-1]
    R, t = absolute_poses(130, K130_SEED + 1)
    pairs = np.concatenate([f.pairs, again])
    keep = (pairs.max(axis=1) < K130_PROTECTED).astype(np.uint8)
    return Family(130, pairs, np.concatenate([f.rt, relative_poses(again, R, t)]), f.bad, keep=keep, **dict(f.params, min_ok=K130_REPEATS_MIN_OK))


# The 24 proper signed permutation matrices (the rotations of a cube): traces 3, 1, 0, -1 for the identity, the quarter turns, the
# third turns and the half turns.
GROUP24 = [np.array(m) for m in (np.eye(3, dtype=np.int64)[list(perm)] * np.array(signs)[:, None]
                                 for perm in itertools.permutations(range(3)) for signs in itertools.product((1, -1), repeat=3))
           if round(np.linalg.det(m)) == 1]
EXACT24_SEED = 24


@functools.lru_cache(maxsize=None)
def exact24():
    """24 sets posed by cube rotations and integer translations in [-8, 8], all 276 pairs in random directions and shuffled, about a
    third of the pairs off by an integer step: every entry, every tr and every e2 is a small integer, exact in every format"""
    rng = np.random.default_rng(EXACT24_SEED)
    pairs = _complete(24, rng)
    R = [GROUP24[g] for g in rng.permutation(24)]
    t = rng.integers(-8, 9, (24, 3))
    rt = np.zeros((276, 12), np.int64)
    for p, (a, b) in enumerate(pairs.tolist()):
        rt[p, :9] = (R[b].T @ R[a]).ravel()
        rt[p, 9:] = R[b].T @ (t[a] - t[b])
    bad = np.sort(rng.choice(276, 92, replace=False))
    for p in bad:
        kind = rng.integers(3)
        if kind == 0:
            rt[p, 9 + rng.integers(3)] += 1
        elif kind == 1:
            rt[p, 9:] += (1, 1, 0)
        else:
            rt[p, :9] = (GROUP24[1 + rng.integers(23)] @ rt[p, :9].reshape(3, 3)).ravel()
    assert (GROUP24[0] == np.eye(3)).all()
    return Family(24, pairs, rt, bad, rot_tol=0.0, trans_tol=0.0)


def exact24_integers():
    """(tp, tq, tr_, tr, e2): every triangle of exact24 and its error in np.int64 arithmetic, by the header's composition — its own
    enumeration of the triangles and none of the fp64 code above"""
    f = exact24()
    rt = f.rt.astype(np.int64)
    assert (rt == f.rt).all()
    where = {tuple(ab): p for p, ab in enumerate(f.pairs.tolist())}

    def T(x, y):  # x -> y, and the pair it comes from
        if (x, y) in where:
            p = where[(x, y)]
            return p, rt[p, :9].reshape(3, 3), rt[p, 9:]
        p = where[(y, x)]
        Rm, tv = rt[p, :9].reshape(3, 3), rt[p, 9:]
        return p, Rm.T, -(Rm.T @ tv)

    out = []
    for a, b, c in itertools.combinations(range(24), 3):
        (p, PR, Pt), (q, QR, Qt), (r, CR_, Ct) = T(a, b), T(b, c), T(c, a)
        MR, Mt = QR @ PR, QR @ Pt + Qt
        ER, Et = CR_ @ MR, CR_ @ Mt + Ct
        out.append((p, q, r, int(np.trace(ER)), int(Et @ Et)))
    out = np.array(out, np.int64)
    return tuple(out[:, k] for k in range(5))


PI32 = float(np.float32(np.pi))  # the float nearest pi, the largest rot_tol the host rules accept: tr_min = -1 + 7.6e-15
# (rot_tol, trans_tol) -> the consistent triangles of exact24, from the integers
EXACT24_CUTS = {(0.0, 0.0): 610, (0.0, 1.0): 884, (0.0, 2.0): 1373, (float(np.float32(np.pi / 2)), 1.0): 929, (PI32, 1.0): 950,
                (float(np.float32(2 * np.pi / 3)), 0.0): 666}


def scaled(f, k):
    """the family with every translation and trans_tol multiplied by 2^k, in float"""
    rt = f.rt.copy()
    rt[:, 9:] = np.ldexp(rt[:, 9:], k).astype(np.float32)
    params = dict(f.params, trans_tol=float(np.ldexp(np.float32(f.params["trans_tol"]), k).astype(np.float32)))
    return Family(f.n_sets, f.pairs, rt, f.bad, keep=f.keep, **params)


FLT_MAX = float(np.finfo(np.float32).max)
HOSTILE24_SEED = 666


@functools.lru_cache(maxsize=None)
def hostile24():
    """k24's list with poses that are no rotations: random finite bit patterns over the whole exponent range and both signs, and a
    few records planted — every entry FLT_MAX on a triangle's three pairs, two of them stored reversed (two inverted poses and a third
    factor: |E.t| near 2^517, and its square is +inf), subnormals, -0.0, and one record that is all zero"""
    f = k24()
    rng = np.random.default_rng(HOSTILE24_SEED)
    bits = rng.integers(0, 1 << 32, (276, 12), dtype=np.uint64).astype(np.uint32)
    bits[(bits >> np.uint32(23)) & np.uint32(0xFF) == 0xFF] ^= np.uint32(1 << 23)  # exponent 255 -> 254: finite
    rt = bits.view(np.float32).copy()
    where = {tuple(ab): p for p, ab in enumerate(f.pairs.tolist())}
    # a triangle a < b < c whose pairs on {a, b} and {b, c} are stored reversed: both are inverted on the way round
    a, b, c = next((a, b, c) for a, b, c in itertools.combinations(range(24), 3) if (b, a) in where and (c, b) in where)
    planted = [where[(b, a)], where[(c, b)], where[(a, c)] if (a, c) in where else where[(c, a)]]
    rt[planted] = FLT_MAX
    free = [p for p in range(276) if p not in planted]
    rt[free[0]] = 0.0  # all zero: finite, so valid
    rt[free[1]] = np.array([1, 0x7FFFFF, 0x80000001, 0x807FFFFF] * 3, np.uint32).view(np.float32)  # subnormals, both signs
    rt[free[2], ::2] = -0.0
    rt[free[3]] = -0.0
    return Family(24, f.pairs, rt, planted, rot_tol=ROT_TOL, trans_tol=TRANS_TOL)


def flt_max_triangle(directions):
    """one_triangle's list with every entry of every pose FLT_MAX"""
    f = one_triangle(directions, True)
    return Family(3, f.pairs, np.full((3, 12), FLT_MAX, np.float32), rot_tol=ROT_TOL, trans_tol=TRANS_TOL)
