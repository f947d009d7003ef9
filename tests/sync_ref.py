"""CPU restatement of sc_pairs_sync (include/saccot.h): the reference the GPU tests compare against bit for bit, and the input
families they share.

The arithmetic is numpy float64 on the exactly widened float32 entries, every product, sum, quotient and square root written out
element by element in the header's order, vectorised over the sets (a numpy ufunc call rounds once per operation; no `@`, no dot, no
einsum: a BLAS may fuse or reorder).  The 64 slots of a set's sum are 64 columns of an array, entry i adds into column i mod 64 in
increasing i, and the fold is the header's: for h = 32 .. 1, columns [0, h) += columns [h, 2h).  The composition, the inverse and the
widening are tests/cycles_ref.py's.  The thresholds are arguments: the GPU tests pass the two values sc_sync_thresholds returns.
Only `sync` is the reference; the families are built with whatever is convenient.  The families of
tests/test_gpu_pairs_sync_range.py stand at the end; `integers` is exact24's and exact_ring's expectation in np.int64, which shares
no code with `sync`.
"""
import functools

import numpy as np

import cycles_ref as CR

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
STATUS = 1  # SC_SYNC_STATUS
UNREACHED = SC_ENOHYP  # the status of a set that was never reached
SET_DTYPE = np.dtype({"names": ["Rt", "status", "known_round", "used", "degenerate", "X"],
                      "formats": [("<f4", (12,)), "<i4", "<u4", "<u4", "<u4", ("<f8", (12,))], "offsets": [0, 48, 52, 56, 60, 64], "itemsize": 160})
PAIR_DTYPE = np.dtype({"names": ["status", "used", "r2", "e2", "reserved"], "formats": ["<i4", "<u4", "<f8", "<f8", ("<u4", (2,))],
                       "offsets": [0, 4, 8, 16, 24], "itemsize": 32})
SUMMARY_DTYPE = np.dtype({"names": ["rounds", "converged", "known", "used", "changed_last", "reserved"],
                          "formats": ["<u4", "<u4", "<u4", "<u4", "<u4", ("<u4", (3,))], "offsets": [0, 4, 8, 12, 16, 20], "itemsize": 32})
SLOTS = 64


def thresholds(rot_tol, trans_tol):
    """(r2_max, e2_max) of the header, from the float32 tolerances"""
    r, t = float(np.float32(rot_tol)), float(np.float32(trans_tol))
    return 2.0 * r * r, t * t


# ---- rot(M), vectorised: M[c] arrays, c = 0 .. 8 row-major -------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _pick(i, rows):
    return [np.where(i == 0, rows[0][r], np.where(i == 1, rows[1][r], rows[2][r])) for r in range(3)]


def rot(M):
    """the header's rot(M) -> R[c] arrays, c = 0 .. 8 row-major; not finite where M's rank is below two"""
    one, zero = np.ones_like(M[0]), np.zeros_like(M[0])
    B = [[M[3 * c + r].copy() for r in range(3)] for c in range(3)]
    V = [[(one if r == c else zero).copy() for r in range(3)] for c in range(3)]
    with np.errstate(all="ignore"):
        for _sweep in range(10):
            for ip, iq in ((0, 1), (0, 2), (1, 2)):
                alpha, beta, gamma = _dot(B[ip], B[ip]), _dot(B[iq], B[iq]), _dot(B[ip], B[iq])
                turn = gamma != 0.0
                zeta = (beta - alpha) / (gamma + gamma)
                tt = 1.0 / (np.abs(zeta) + np.sqrt(zeta * zeta + 1.0))
                tt = np.where(zeta < 0.0, -tt, tt)
                cs = 1.0 / np.sqrt(tt * tt + 1.0)
                sn = cs * tt
                for W in (B, V):
                    for r in range(3):
                        x, y = W[ip][r], W[iq][r]
                        W[ip][r] = np.where(turn, cs * x - sn * y, x)
                        W[iq][r] = np.where(turn, sn * x + cs * y, y)
        n = [_dot(B[c], B[c]) for c in range(3)]
        i1 = np.zeros(M[0].shape, np.int64); m1 = n[0]
        i1 = np.where(n[1] > m1, 1, i1); m1 = np.where(n[1] > m1, n[1], m1)
        i1 = np.where(n[2] > m1, 2, i1)
        i2 = np.where(i1 == 0, 1, 0)
        c = 3 - i1 - i2
        nc = np.where(c == 0, n[0], np.where(c == 1, n[1], n[2]))
        ni2 = np.where(i2 == 0, n[0], np.where(i2 == 1, n[1], n[2]))
        i2 = np.where(nc > ni2, c, i2)
        b1, b2, v1, v2 = _pick(i1, B), _pick(i2, B), _pick(i1, V), _pick(i2, V)
        s1, s2 = np.sqrt(_dot(b1, b1)), np.sqrt(_dot(b2, b2))
        u1, u2 = [b1[r] / s1 for r in range(3)], [b2[r] / s2 for r in range(3)]
        u3, v3 = _cross(u1, u2), _cross(v1, v2)
        return [(v1[r] * u1[c] + v2[r] * u2[c]) + v3[r] * u3[c] for r in range(3) for c in range(3)]


def _sq_left_to_right(d):
    s = d[0] * d[0]
    for x in d[1:]:
        s = s + x * x
    return s


def _flat(T):
    """a transform (R[i][j], t[i]) as its twelve components: R row-major, then t"""
    return [T[0][i][j] for i in range(3) for j in range(3)] + [T[1][i] for i in range(3)]


def _unflat(X, idx=slice(None)):
    return [[X[3 * i + j][idx] for j in range(3)] for i in range(3)], [X[9 + i][idx] for i in range(3)]


def adjacency(pairs):
    """every set's sorted list, flattened: (set, neighbour, pair, index in the set's list), ordered by (set, neighbour, pair)"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    p = np.flatnonzero(pairs[:, 0] != pairs[:, 1])
    s, n, pp = np.concatenate([pairs[p, 0], pairs[p, 1]]), np.concatenate([pairs[p, 1], pairs[p, 0]]), np.concatenate([p, p])
    order = np.lexsort((pp, n, s))
    s, n, pp = s[order], n[order], pp[order]
    start = np.searchsorted(s, s, side="left")
    return s, n, pp, np.arange(len(s)) - start


def sync(n_sets, pairs, rt, r2_max, e2_max, anchor=0, max_rounds=32, use=None, weight=None, statuses=None, trace=None):
    """-> (sets (n_sets,) of SET_DTYPE, pairs (P,) of PAIR_DTYPE, summary: one record of SUMMARY_DTYPE).  use: None or a word per
    pair; weight: None or a float32 per pair; statuses: the int32 at byte 48 of every record (SC_SYNC_STATUS), or None.  trace: a
    list that receives, per round run, (changed (n_sets,) bool, dR2, dt2, updated (n_sets,) bool)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P = len(pairs)
    assert pairs.max() < n_sets and anchor < n_sets
    rt = np.asarray(rt, np.float32).reshape(P, 12)
    status = np.zeros(P, np.int32) if statuses is None else np.asarray(statuses, np.int32).copy()
    status[(status == SC_OK) & ~np.isfinite(rt).all(axis=1)] = SC_EINVAL
    edge = (status == SC_OK) & (pairs[:, 0] != pairs[:, 1])
    w = np.ones(P) if weight is None else np.asarray(weight, np.float32).reshape(P).astype(np.float64)  # exact
    with np.errstate(invalid="ignore"):
        usable = edge & (np.ones(P, bool) if use is None else np.asarray(use).reshape(P) != 0) & np.isfinite(w) & (w > 0)
    safe = np.where(edge[:, None], rt, 0).astype(np.float32)  # (what is no edge is never composed)
    stored = CR._widen(safe)
    inv = CR._inverse(*stored)
    fwd = pairs[:, 0] < pairs[:, 1]  # stored (lower, higher)
    up, down = CR._where(fwd, stored, inv), CR._where(fwd, inv, stored)  # lower -> higher, higher -> lower
    es, en, ep, ei = adjacency(pairs)
    TE = CR._where(es < en, CR._take(up, ep), CR._take(down, ep))  # T_p(s -> n) of every entry
    slot, trip = ei % SLOTS, ei // SLOTS
    trips = int(trip.max()) + 1 if len(trip) else 0
    ew, e_usable = w[ep], usable[ep] & (es != anchor)  # (the anchor is never recomputed)

    X = [np.zeros(n_sets) for _ in range(12)]
    for c in (0, 4, 8):
        X[c][anchor] = 1.0
    known = np.zeros(n_sets, bool); known[anchor] = True
    known_round, used, degenerate = np.zeros(n_sets, np.uint32), np.zeros(n_sets, np.uint32), np.zeros(n_sets, np.uint32)
    K, converged, changed_last = max_rounds, 0, 0
    for k in range(1, max_rounds + 1):
        live = e_usable & known[en]
        with np.errstate(all="ignore"):
            Pk = _flat(CR._compose(_unflat(X, en), TE))
            acc = [np.zeros((n_sets, SLOTS)) for _ in range(13)]
            for t in range(trips):  # increasing i: a (set, slot) is met once a trip
                m = live & (trip == t)
                for c in range(12):
                    acc[c][es[m], slot[m]] = acc[c][es[m], slot[m]] + ew[m] * Pk[c][m]
                acc[12][es[m], slot[m]] = acc[12][es[m], slot[m]] + ew[m]
            h = SLOTS // 2
            while h:
                for c in range(13):
                    acc[c][:, :h] = acc[c][:, :h] + acc[c][:, h:2 * h]
                h //= 2
            count = np.bincount(es[live], minlength=n_sets)
            new = rot([acc[c][:, 0] for c in range(9)]) + [acc[9 + c][:, 0] / acc[12][:, 0] for c in range(3)]
            finite = np.logical_and.reduce([np.isfinite(x) for x in new])
            update = (count > 0) & finite
            dR2 = _sq_left_to_right([new[c] - X[c] for c in range(9)])
            dt2 = _sq_left_to_right([new[9 + c] - X[9 + c] for c in range(3)])
            changed = update & (~known | (dR2 > r2_max) | (dt2 > e2_max))
        used = count.astype(np.uint32)
        degenerate = degenerate + ((count > 0) & ~finite).astype(np.uint32)
        known_round = np.where(update & ~known, k, known_round).astype(np.uint32)
        X = [np.where(update, new[c], X[c]) for c in range(12)]
        known = known | update
        if trace is not None:
            trace.append((changed, dR2, dt2, update))
        changed_last = int(changed.sum())
        if changed_last == 0:
            K, converged = k, 1
            break

    sets = np.zeros(n_sets, SET_DTYPE)
    Xa = np.stack(X, axis=1)
    sets["X"] = Xa
    with np.errstate(over="ignore"):  # a component past FLT_MAX rounds to an infinity
        sets["Rt"] = Xa.astype(np.float32)
    sets["status"] = np.where(known, SC_OK, UNREACHED)
    sets["known_round"], sets["used"], sets["degenerate"] = known_round, used, degenerate
    res = np.zeros(P, PAIR_DTYPE)
    res["status"] = status
    a, b = pairs[:, 0], pairs[:, 1]
    pair_used = usable & known[a] & known[b]
    with np.errstate(all="ignore"):
        Q = _flat(CR._compose(_unflat(X, b), stored))
        r2 = _sq_left_to_right([X[c][a] - Q[c] for c in range(9)])
        e2 = _sq_left_to_right([X[9 + c][a] - Q[9 + c] for c in range(3)])
    res["used"] = pair_used
    res["r2"], res["e2"] = np.where(pair_used, r2, 0.0), np.where(pair_used, e2, 0.0)
    summary = np.zeros(1, SUMMARY_DTYPE)
    summary["rounds"], summary["converged"], summary["known"], summary["used"], summary["changed_last"] = K, converged, known.sum(), pair_used.sum(), changed_last
    return sets, res, summary[0]


# ---- the input families ---------------------------------------------------------------------------------------------------------------
TOL = 1e-4  # the tolerances (radians, length units) the families are used with unless a test says otherwise
NOISE_DEG, NOISE_TRANS = 0.3, 3e-3


class Family:
    def __init__(self, n_sets, pairs, rt, R=None, t=None, **params):
        self.n_sets, self.pairs, self.rt = n_sets, np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2), np.ascontiguousarray(rt, np.float32)
        self.R, self.t = R, t  # the absolute poses the list was made from, where there are any
        self.params = dict(dict(rot_tol=TOL, trans_tol=TOL), **params)
        self.use = self.weight = self.statuses = None  # per pair, where a family brings them


def truth(f, anchor=0):
    """(n_sets, 12) float64: every set's pose in the anchor's frame, from the absolute poses the family was made from"""
    out = np.zeros((f.n_sets, 12))
    for s in range(f.n_sets):
        out[s, :9] = (f.R[anchor].T @ f.R[s]).ravel()
        out[s, 9:] = f.R[anchor].T @ (f.t[s] - f.t[anchor])
    return out


def noisy(rt, seed, deg=NOISE_DEG, trans=NOISE_TRANS):
    """every pose followed by a small rigid motion: a turn of 0 .. deg degrees about a random axis and a shift of length 0 .. trans"""
    rng = np.random.default_rng(seed)
    out = np.asarray(rt, np.float64).copy()
    for p in range(len(out)):
        N = CR.rotation(rng.normal(size=3), np.deg2rad(rng.uniform(0, deg)))
        d = rng.normal(size=3)
        d *= rng.uniform(0, trans) / np.linalg.norm(d)
        out[p, :9] = (N @ out[p, :9].reshape(3, 3)).ravel()
        out[p, 9:] = N @ out[p, 9:] + d
    return out.astype(np.float32)


def errors(sets, f, anchor=0):
    """(largest Frobenius distance of a rotation from the truth, largest distance of a translation) over the sets"""
    d = sets["X"] - truth(f, anchor)
    return float(np.sqrt((d[:, :9] ** 2).sum(axis=1)).max()), float(np.sqrt((d[:, 9:] ** 2).sum(axis=1)).max())


@functools.lru_cache(maxsize=None)
def k24(noise=True):
    """cycles_ref.k24's list — 24 sets, all 276 pairs in random stored directions, shuffled — with the poses of one world, noisy or exact"""
    pairs = CR.k24().pairs
    R, t = CR.absolute_poses(24, CR.K24_SEED + 1)
    rt = CR.relative_poses(pairs, R, t)
    return Family(24, pairs, noisy(rt, 241) if noise else rt, R, t)


@functools.lru_cache(maxsize=None)
def k24_repeats():
    """cycles_ref.k24_repeats's list (four pairs twice, three of them also reversed), noisy: every copy has a noise of its own"""
    pairs = CR.k24_repeats().pairs
    R, t = CR.absolute_poses(24, CR.K24_SEED + 1)
    return Family(24, pairs, noisy(CR.relative_poses(pairs, R, t), 242), R, t)


@functools.lru_cache(maxsize=None)
def g512(noise=True):
    """512 sets, every set the source of ten pairs to random other sets, no two sets paired twice: about 20 pairs a set, 5120 pairs"""
    rng = np.random.default_rng(512)
    seen, pairs = set(), []
    for s in range(512):
        while sum(1 for a, _b in pairs if a == s) < 10:
            n = (s + 1 + int(rng.integers(511))) % 512
            if (min(s, n), max(s, n)) not in seen:
                seen.add((min(s, n), max(s, n)))
                pairs.append((s, n))
    pairs = np.array(pairs)
    pairs = pairs[rng.permutation(len(pairs))]
    R, t = CR.absolute_poses(512, 513)
    rt = CR.relative_poses(pairs, R, t)
    return Family(512, pairs, noisy(rt, 514) if noise else rt, R, t)


@functools.lru_cache(maxsize=None)
def chain(n=42):
    """n sets in a row and nothing else: pairs (i, i + 1), every other one stored reversed"""
    pairs = np.array([(i, i + 1) if i % 2 else (i + 1, i) for i in range(n - 1)])
    R, t = CR.absolute_poses(n, 42)
    return Family(n, pairs, CR.relative_poses(pairs, R, t), R, t)


@functools.lru_cache(maxsize=None)
def hub(n=300):
    """cycles_ref.hub's list at n sets — set 0 paired with every other set, ring pairs among the others —, noisy: set 0's sorted list
    has n - 1 entries"""
    pairs = CR.hub(n).pairs
    R, t = CR.absolute_poses(n, 11)
    return Family(n, pairs, noisy(CR.relative_poses(pairs, R, t), 301), R, t)


WIDE_SETS = 8200  # more sets than the round kernel's grid has waves (2048 workgroups x 4)


@functools.lru_cache(maxsize=None)
def wide(n=WIDE_SETS):
    """n sets on a ring with the chords (i, i + 97) and a spoke from set 0 to every 16th set: every set is reached within a few
    rounds, and the sets past one trip of the round kernel's grid loop among them"""
    ring = [(i, (i + 1) % n) for i in range(n)]
    chords = [((i + 97) % n, i) for i in range(n)]
    spokes = [(0, i) for i in range(16, n, 16)]
    pairs = np.array(ring + chords + spokes)
    R, t = CR.absolute_poses(n, 8200)
    return Family(n, pairs, noisy(CR.relative_poses(pairs, R, t), 8201), R, t, max_rounds=12)


@functools.lru_cache(maxsize=None)
def two_components():
    """k24 beside a second world of 6 sets (24 .. 29, all pairs) that no pair joins to the first"""
    f = k24()
    more = np.array([(a, b) for a in range(24, 30) for b in range(a + 1, 30)])
    R2, t2 = CR.absolute_poses(6, 66)
    rt2 = CR.relative_poses(more - 24, R2, t2)
    return Family(30, np.concatenate([f.pairs, more]), np.concatenate([f.rt, rt2]), list(f.R) + list(R2), np.concatenate([f.t, t2]))


def degenerate():
    """sets 2 and 3 beside the anchor, set 1 beside both: its two predictions are I and diag(1, -1, -1), whose sum has rank one"""
    I = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    half = [1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0]
    return Family(4, [(2, 0), (3, 0), (1, 2), (1, 3)], np.array([I, I, I, half], np.float32))


# The cut family.  cycles_ref.exact24's world before its corruption — cube rotations, integer translations, all 276 pairs —: every
# sum of the method is a sum of small integers and every quotient exact, so the rounds are exact.  Set CUT_SET may use two of its
# pairs only, the one to the anchor and the one to CUT_NEAR, and the record of the first is off by 2^-3 in one translation component.
# Round 1 places CUT_SET by the anchor alone, 2^-3 off; round 2 averages two predictions, one of them exact: the set moves by exactly
# 2^-4, dt2 = 2^-8 = e2_max at trans_tol = 2^-4.
CUT_SET, CUT_NEAR, CUT_STEP, CUT_TOL = 5, 9, 2.0 ** -3, 2.0 ** -4


def _exact_world():
    """(pairs, R, t) of cycles_ref.exact24 before its corruption, from its draws in its order: all 276 pairs in random stored
    directions and shuffled, 24 cube rotations and integer translations in [-8, 8], as np.int64"""
    rng = np.random.default_rng(CR.EXACT24_SEED)
    pairs = CR._complete(24, rng)
    R = [CR.GROUP24[g] for g in rng.permutation(24)]
    return pairs, R, rng.integers(-8, 9, (24, 3))


def _exact_records(pairs, R, t):
    rt = np.zeros((len(pairs), 12))
    for p, (a, b) in enumerate(pairs.tolist()):
        rt[p, :9] = (R[b].T @ R[a]).ravel()
        rt[p, 9:] = R[b].T @ (t[a] - t[b])
    return rt


@functools.lru_cache(maxsize=None)
def cut24():
    pairs, R, t = _exact_world()
    rt = _exact_records(pairs, R, t)
    use = np.ones(276, np.uint32)
    for p, (a, b) in enumerate(pairs.tolist()):
        if CUT_SET in (a, b):
            other = a + b - CUT_SET
            use[p] = other in (0, CUT_NEAR)
            if other == 0:
                rt[p, 9] += CUT_STEP
    f = Family(24, pairs, rt, R, t.astype(np.float64), rot_tol=0.0, trans_tol=CUT_TOL)
    f.use = use
    return f


# ---- the families of the range tests: on the rotation cut, exact in integers, at the ends of the number range, to the round limit ---
# (tests/test_sync_abi.py asserts what the reference measures on them, as literals)

# The rotation cut.  Round 1 places sets 1, 2 and 3 at the identity by the anchor alone.  In round 2 set 1 sums I + 2 diag(1, -1, -1)
# = diag(3, -1, -1): orthogonal rows, no Jacobi turn, rot gives diag(1, -1, -1) exactly and dR2 = 8.0 = r2_max at rot_tol 2.0.  Sets 2
# and 3 sum I + diag(1, -1, -1) = diag(2, 0, 0), of rank one: known sets that meet a degenerate sum and keep their pose.
RCUT_TOL = 2.0


@functools.lru_cache(maxsize=None)
def rcut():
    I = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    half = [1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0]
    return Family(4, [(1, 0), (2, 0), (3, 0), (1, 2), (1, 3)], np.array([I, I, I, half, half], np.float32), rot_tol=RCUT_TOL, trans_tol=0.0)


@functools.lru_cache(maxsize=None)
def exact24(anchor=0):
    """cut24's world with nothing corrupted and every pair usable: every prediction of a set is the truth, a sum of k equal signed
    permutation matrices has orthogonal rows and k t / k is exact, so every round is exact"""
    pairs, R, t = _exact_world()
    return Family(24, pairs, _exact_records(pairs, R, t), R, t, rot_tol=0.0, trans_tol=0.0, anchor=anchor)


@functools.lru_cache(maxsize=None)
def exact_ring():
    """the same 24 absolute poses, the ring pairs (i, i + 1 mod 24) only, every other one stored reversed"""
    _all, R, t = _exact_world()
    pairs = np.array([(i, (i + 1) % 24) if i % 2 else ((i + 1) % 24, i) for i in range(24)])
    return Family(24, pairs, _exact_records(pairs, R, t), R, t, rot_tol=0.0, trans_tol=0.0)


def integers(f, anchor=0):
    """(n_sets, 12) np.int64: every set's pose in the anchor's frame from the integer absolute poses, in integer arithmetic — none
    of the reference's code"""
    out = np.zeros((f.n_sets, 12), np.int64)
    Ra, ta = np.asarray(f.R[anchor], np.int64), np.asarray(f.t[anchor], np.int64)
    for s in range(f.n_sets):
        out[s, :9] = (Ra.T @ np.asarray(f.R[s], np.int64)).ravel()
        out[s, 9:] = Ra.T @ (np.asarray(f.t[s], np.int64) - ta)
    return out


SCALES_EXACT = (-100, -60, 60, 100, 120)  # 2^k of these leaves every translation of k24 and TOL a normal float: exact
SCALE_UNDER = -140  # trans_tol becomes 0.0 and translations go subnormal: rounded


@functools.lru_cache(maxsize=None)
def scaled(k, noise=True):
    """k24 with every translation and trans_tol multiplied by 2^k, in float (cycles_ref.scaled's rule)"""
    f = k24(noise)
    rt = f.rt.copy()
    rt[:, 9:] = np.ldexp(rt[:, 9:], k).astype(np.float32)
    return Family(f.n_sets, f.pairs, rt, f.R, f.t, rot_tol=TOL, trans_tol=float(np.ldexp(np.float32(TOL), k).astype(np.float32)))


WEIGHT_SEED = 2401


@functools.lru_cache(maxsize=None)
def weight_scaled(k):
    """k24 with one fixed weight vector, 1 .. 2 times 2^-20 .. 2^20, multiplied by 2^k in float"""
    rng = np.random.default_rng(WEIGHT_SEED)
    f = k24()
    g = Family(f.n_sets, f.pairs, f.rt, f.R, f.t)
    g.weight = np.ldexp(np.ldexp(rng.uniform(1, 2, 276), rng.integers(-20, 21, 276)).astype(np.float32), k).astype(np.float32)
    return g


FLT_MAX = np.float32(CR.FLT_MAX)
WEIGHTS_RANGE_PLANTED = {7: np.float32(1e-45), 19: FLT_MAX, 101: np.float32(-0.0), 202: np.float32(0.0)}  # pair -> weight


@functools.lru_cache(maxsize=None)
def weights_range():
    """k24 with weights over the whole fp32 range, 1 .. 2 times 2^-149 .. 2^127, and four planted: the smallest subnormal, FLT_MAX and
    both zeros (which are not greater than 0: those two pairs are not usable)"""
    rng = np.random.default_rng(WEIGHT_SEED + 1)
    f = k24()
    g = Family(f.n_sets, f.pairs, f.rt, f.R, f.t)
    g.weight = np.ldexp(rng.uniform(1, 2, 276), rng.integers(-149, 128, 276)).astype(np.float32)
    for p, w in WEIGHTS_RANGE_PLANTED.items():
        g.weight[p] = w
    return g


@functools.lru_cache(maxsize=None)
def hostile():
    """cycles_ref.hostile24's records — random finite bit patterns over the whole exponent range, a FLT_MAX triangle, subnormals, -0.0
    and an all-zero record — as the poses of k24's list"""
    f = CR.hostile24()
    return Family(24, f.pairs, f.rt)


RING40_SEED = 40


@functools.lru_cache(maxsize=None)
def ring40():
    """the header's bare ring: 40 noisy sets, the pairs (i, i + 1 mod 40) and nothing else.  It diffuses."""
    pairs = np.array([(i, (i + 1) % 40) for i in range(40)])
    R, t = CR.absolute_poses(40, RING40_SEED)
    return Family(40, pairs, noisy(CR.relative_poses(pairs, R, t), RING40_SEED + 1), R, t, max_rounds=256)


@functools.lru_cache(maxsize=None)
def sparse(n=WIDE_SETS):
    """chain()'s 41 pairs among n sets: all but 42 of the sets have empty lists, and the sets past one trip of the round kernel's
    grid loop have nothing to do"""
    f = chain()
    return Family(n, f.pairs, f.rt, max_rounds=64)


def self_star(sets, anchor):
    """a first call's set records as the pose records of a second: the pairs (s, anchor) for every s — the anchor's a self pair —,
    pair s's record the 160 bytes of set s, whose Rt maps s onto the anchor and whose status stands at byte 48"""
    n = len(sets)
    g = Family(n, np.stack([np.arange(n), np.full(n, anchor)], axis=1), sets["Rt"], anchor=anchor, flags=STATUS)
    g.statuses = sets["status"].astype(np.int32)
    return g
