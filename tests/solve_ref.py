"""CPU restatement of sc_pairs_solve (include/saccot.h): the reference the GPU tests compare against bit for bit, and the input
families they share.

The arithmetic is numpy float64, every product, sum, difference and quotient written out element by element in the header's order,
vectorised over the pairs, the entries or the sets (a numpy ufunc call rounds once per operation; no `@`, no dot, no einsum: a BLAS
may fuse or reorder).  The 64 slots of a row sum are 64 columns of an array, entry i adds into column i mod 64 in increasing i, the
fold is the header's; a grand sum is 64 columns summed left to right per chunk, then the chunk sums one after the other.  The
composition, the inverse and the widening are tests/cycles_ref.py's, rot(M) and the sorted lists tests/sync_ref.py's.  The
thresholds are arguments: the GPU tests pass the three values sc_solve_thresholds returns.
Only `solve` is the reference; the families are built with whatever is convenient.
"""
import functools

import numpy as np

import cycles_ref as CR
import sync_ref as SR

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
STATUS, INFO_STATUS = 1, 2  # SC_SOLVE_STATUS, SC_SOLVE_INFO_STATUS
FREE, ANCHOR, UNKNOWN, ISOLATED = 0, 1, 2, 3
CONVERGED, ROSE, MAX_OUTER = 1, 2, 3
SET_DTYPE = np.dtype({"names": ["Rt", "status", "state", "degenerate", "reserved", "X"],
                      "formats": [("<f4", (12,)), "<i4", "<u4", "<u4", "<u4", ("<f8", (12,))], "offsets": [0, 48, 52, 56, 60, 64], "itemsize": 160})
PAIR_DTYPE = np.dtype({"names": ["status", "used", "cost", "w2", "v2", "reserved"], "formats": ["<i4", "<u4", "<f8", "<f8", "<f8", ("<u4", (4,))],
                       "offsets": [0, 4, 8, 16, 24, 32], "itemsize": 48})
SUMMARY_DTYPE = np.dtype({"names": ["outer", "stop", "inner_total", "inner_last", "free_sets", "used_pairs", "held_last", "reserved", "cost0", "cost", "rz0",
                                    "reserved2"],
                          "formats": ["<u4"] * 8 + ["<f8"] * 4, "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56], "itemsize": 64})
INFO_DTYPE = np.dtype({"names": ["info", "sse", "status", "inliers", "reserved"], "formats": [("<f8", (36,)), "<f8", "<i4", "<u4", ("<u4", (4,))],
                       "offsets": [0, 288, 296, 300, 304], "itemsize": 320})  # sc_pose_info_result
SLOTS = 64


def thresholds(rot_tol, trans_tol, cg_tol):
    """(r2_max, e2_max, cg2) of the header, from the float32 parameters"""
    c = float(np.float32(cg_tol))
    return SR.thresholds(rot_tol, trans_tol) + (c * c,)


def _seq(terms):
    """sum_k a_k, left to right"""
    s = terms[0]
    for x in terms[1:]:
        s = s + x
    return s


def _dot6(a, b):
    return _seq([a[c] * b[c] for c in range(6)])


def _grand(v):
    """the header's grand sum of a value per set (or per pair)"""
    n = len(v)
    nch = (n + SLOTS - 1) // SLOTS
    m = np.zeros(nch * SLOTS)
    m[:n] = v
    m = m.reshape(nch, SLOTS)
    s = np.zeros(nch)
    for k in range(SLOTS):
        s = s + m[:, k]
    t = np.float64(0.0)
    for k in range(nch):
        t = t + s[k]
    return t


class _Rows:
    """the header's row sums over every set's sorted list: 64 slots, entry i into slot i mod 64 in increasing i, folded"""

    def __init__(self, n_sets, pairs, usable):
        self.n = n_sets
        self.es, self.en, self.ep, ei = SR.adjacency(pairs)
        self.slot, self.trip = ei % SLOTS, ei // SLOTS
        self.trips = int(self.trip.max()) + 1 if len(self.trip) else 0
        self.live = usable[self.ep]
        self.forward = pairs[self.ep, 0] == self.es  # the set is the pair's stored first
        self.masks = [np.flatnonzero(self.live & (self.trip == t)) for t in range(self.trips)]

    def sum(self, terms, subtract=None):
        """terms: per component an array over the entries -> per component the sets' slot 0.  subtract: entries that subtract"""
        out = []
        for v in terms:
            acc = np.zeros((self.n, SLOTS))
            for m in self.masks:  # increasing i: a (set, slot) is met once a trip
                s, k = self.es[m], self.slot[m]
                acc[s, k] = acc[s, k] + v[m] if subtract is None else np.where(subtract[m], acc[s, k] - v[m], acc[s, k] + v[m])
            h = SLOTS // 2
            while h:
                acc[:, :h] = acc[:, :h] + acc[:, h:2 * h]
                h //= 2
            out.append(acc[:, 0].copy())
        return out


def _factor(H):
    """H[i][j], i <= j, arrays over the sets -> (L[i][k], D[i], held)"""
    Hm = [[H[min(i, j)][max(i, j)] for j in range(6)] for i in range(6)]
    L = [[None] * 6 for _ in range(6)]
    D = [None] * 6
    held = np.zeros(Hm[0][0].shape, bool)
    for j in range(6):
        u = [L[j][k] * D[k] for k in range(j)]
        a = Hm[j][j]
        for k in range(j):
            a = a - L[j][k] * u[k]
        D[j] = a
        held = held | ~((a > 0.0) & (a < np.inf))
        for i in range(j + 1, 6):
            b = Hm[i][j]
            for k in range(j):
                b = b - L[i][k] * u[k]
            L[i][j] = b / a
    return L, D, held


def _solve6(L, D, r):
    y = [None] * 6
    for i in range(6):
        a = r[i]
        for k in range(i):
            a = a - L[i][k] * y[k]
        y[i] = a
    z = [None] * 6
    for i in range(5, -1, -1):
        a = y[i] / D[i]
        for k in range(i + 1, 6):
            a = a - L[k][i] * z[k]
        z[i] = a
    return z


def _errors(X, a, b, Tinv, info, usable):
    """every pair's xi, y, cost, w2, v2 at state X (zeros where the pair is not usable), and X(b)"""
    Xa, Xb = SR._unflat(X, a), SR._unflat(X, b)
    E = CR._compose(CR._compose(CR._inverse(*Xb), Xa), Tinv)
    ER, Et = E
    xi = [(ER[2][1] - ER[1][2]) / 2.0, (ER[0][2] - ER[2][0]) / 2.0, (ER[1][0] - ER[0][1]) / 2.0, Et[0], Et[1], Et[2]]
    y = [_seq([info[6 * i + k] * xi[k] for k in range(6)]) for i in range(6)]
    cost = _dot6(xi, y)
    w2 = (xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]
    v2 = (xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]
    zero = np.zeros(len(a))
    return xi, y, np.where(usable, cost, zero), np.where(usable, w2, zero), np.where(usable, v2, zero), Xb


def _linearise(Xb, info, y):
    """W[i][c] (i <= c) and g[i] of every pair from X(b), its info and y"""
    R, t = Xb
    zero = np.zeros(R[0][0].shape)
    A = [[None] * 6 for _ in range(6)]
    for i in range(3):
        c = [R[0][i], R[1][i], R[2][i]]
        ct = SR._cross(c, t)
        for k in range(3):
            A[i][k] = c[k]; A[3 + i][3 + k] = c[k]
            A[i][3 + k] = zero
            A[3 + i][k] = -ct[k]
    M = [[_seq([info[6 * i + k] * A[k][c] for k in range(6)]) for c in range(6)] for i in range(6)]
    W = [[_seq([A[k][i] * M[k][c] for k in range(6)]) if c >= i else None for c in range(6)] for i in range(6)]
    g = [_seq([A[k][i] * y[k] for k in range(6)]) for i in range(6)]
    return W, g


def solve(n_sets, pairs, rt, init_X, init_status, r2_max, e2_max, cg2, anchor=0, max_outer=8, max_inner=64, use=None, info=None,
          info_statuses=None, statuses=None, trace=None):
    """-> (sets (n_sets,) of SET_DTYPE, pairs (P,) of PAIR_DTYPE, summary: one record of SUMMARY_DTYPE).  init_X (n_sets, 12) float64,
    init_status (n_sets,) int32; use: None or a word per pair; info: None or (P, 36) float64; info_statuses: the int32 at byte 296 of
    every info record (SC_SOLVE_INFO_STATUS), or None; statuses: the int32 at byte 48 of every pose record (SC_SOLVE_STATUS), or None.
    trace: a list that receives, per step taken, a dict (cost, inner, rz0, held, changed)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P = len(pairs)
    assert pairs.max() < n_sets and anchor < n_sets
    rt = np.asarray(rt, np.float32).reshape(P, 12)
    init_X = np.asarray(init_X, np.float64).reshape(n_sets, 12)
    init_status = np.asarray(init_status, np.int32).reshape(n_sets)
    status = np.zeros(P, np.int32) if statuses is None else np.asarray(statuses, np.int32).copy()
    status[(status == SC_OK) & ~np.isfinite(rt).all(axis=1)] = SC_EINVAL
    edge = (status == SC_OK) & (pairs[:, 0] != pairs[:, 1])
    known = (init_status == SC_OK) & np.isfinite(init_X).all(axis=1)
    a, b = pairs[:, 0], pairs[:, 1]
    if info is None:
        infoa = np.tile(np.eye(6).ravel(), (P, 1))
        info_ok = np.ones(P, bool)
    else:
        infoa = np.asarray(info, np.float64).reshape(P, 36)
        info_ok = np.isfinite(infoa).all(axis=1) & (np.ones(P, bool) if info_statuses is None else np.asarray(info_statuses).reshape(P) == SC_OK)
    usable = edge & (np.ones(P, bool) if use is None else np.asarray(use).reshape(P) != 0) & info_ok & known[a] & known[b]
    infoc = [np.where(usable, infoa[:, c], 0.0) for c in range(36)]  # (what is not usable is computed on zeros and thrown away)
    safe = np.where(edge[:, None], rt, 0).astype(np.float32)
    Tinv = CR._inverse(*CR._widen(safe))  # T_p(b -> a)
    deg = np.bincount(np.concatenate([a[usable], b[usable]]), minlength=n_sets)
    state = np.where(~known, UNKNOWN, np.where(np.arange(n_sets) == anchor, ANCHOR, np.where(deg == 0, ISOLATED, FREE))).astype(np.uint32)
    free = state == FREE
    rows = _Rows(n_sets, pairs, usable)
    es, en, ep = rows.es, rows.en, rows.ep

    Xsafe = np.where(known[:, None], init_X, 0.0)  # (an unknown set's X is never computed on; it is passed through below)
    X = [Xsafe[:, c].copy() for c in range(12)]
    degenerate = np.zeros(n_sets, np.uint32)
    with np.errstate(all="ignore"):
        xi, y, cost_p, w2, v2, Xb = _errors(X, a, b, Tinv, infoc, usable)
        costs = [_grand(cost_p)]
        err = (cost_p, w2, v2)
        K, J, stop = 0, 0, 0
        inner, helds, rz0s = [0], [0], [np.float64(0.0)]
        if not free.any():
            stop = CONVERGED
        j = 0
        while not stop:
            j += 1
            W, g = _linearise(Xb, infoc, y)
            G = rows.sum([g[c][ep] for c in range(6)], subtract=~rows.forward)
            Hd = rows.sum([W[i][c][ep] for i in range(6) for c in range(i, 6)])
            H = [[None] * 6 for _ in range(6)]
            at = 0
            for i in range(6):
                for c in range(i, 6):
                    H[i][c] = Hd[at]; at += 1
            L, D, held = _factor(H)
            held = held & free
            active = free & ~held
            degenerate = degenerate + held.astype(np.uint32)
            zero = np.zeros(n_sets)

            def precond(r):
                z = _solve6(L, D, r)
                return [np.where(active, z[c], zero) for c in range(6)]

            Wfull = [[W[min(i, c)][max(i, c)][ep] for c in range(6)] for i in range(6)]
            x = [zero.copy() for _ in range(6)]
            r = [np.where(free, -G[c], zero) for c in range(6)]
            z = precond(r)
            rz = [_grand(np.where(active, _dot6(r, z), zero))]
            n_inner = 0
            p = None
            if rz[0] != 0.0:
                for i in range(1, max_inner + 1):
                    if i == 1:
                        p = [z[c].copy() for c in range(6)]
                    else:
                        beta = rz[i - 1] / rz[i - 2]
                        p = [np.where(active, z[c] + beta * p[c], zero) for c in range(6)]
                    d = [p[c][es] - p[c][en] for c in range(6)]
                    q = rows.sum([_seq([Wfull[i_][c] * d[c] for c in range(6)]) for i_ in range(6)])
                    pq = _grand(np.where(active, _dot6(p, q), zero))
                    if not (pq > 0.0 and pq < np.inf):
                        break
                    alpha = rz[i - 1] / pq
                    x = [np.where(active, x[c] + alpha * p[c], x[c]) for c in range(6)]
                    r = [np.where(active, r[c] - alpha * q[c], r[c]) for c in range(6)]
                    z = precond(r)
                    rz.append(_grand(np.where(active, _dot6(r, z), zero)))
                    n_inner = i
                    if rz[i] <= cg2 * rz[0]:
                        break
            # the step
            one = np.ones(n_sets)
            Q = SR.rot([one, -x[2], x[1], x[2], one, -x[0], -x[1], x[0], one])
            Mn = CR._compose(([[Q[3 * i_ + c] for c in range(3)] for i_ in range(3)], [x[3], x[4], x[5]]), SR._unflat(X))
            new = SR.rot([Mn[0][i_][c] for i_ in range(3) for c in range(3)]) + [Mn[1][c] for c in range(3)]
            finite = np.logical_and.reduce([np.isfinite(v) for v in new])
            take = active & finite
            degenerate = degenerate + (active & ~finite).astype(np.uint32)
            dR2 = SR._sq_left_to_right([new[c] - X[c] for c in range(9)])
            dt2 = SR._sq_left_to_right([new[9 + c] - X[9 + c] for c in range(3)])
            changed = take & ((dR2 > r2_max) | (dt2 > e2_max))
            Xn = [np.where(take, new[c], X[c]) for c in range(12)]
            xi, y, cost_p, w2n, v2n, Xbn = _errors(Xn, a, b, Tinv, infoc, usable)
            c_new = _grand(cost_p)
            J = j
            inner.append(n_inner); helds.append(int(held.sum())); rz0s.append(rz[0])
            if trace is not None:
                trace.append(dict(cost=float(c_new), inner=n_inner, rz0=float(rz[0]), held=int(held.sum()), changed=int(changed.sum())))
            if not (c_new <= costs[j - 1]):
                K, stop = j - 1, ROSE
                break
            costs.append(c_new)
            X, Xb, err, K = Xn, Xbn, (cost_p, w2n, v2n), j
            if int(changed.sum()) == 0 or rz[0] == 0.0:
                stop = CONVERGED
            elif j == max_outer:
                stop = MAX_OUTER

    sets = np.zeros(n_sets, SET_DTYPE)
    Xa = np.where(known[:, None], np.stack(X, axis=1), init_X)  # an unknown set's X, NaNs and all
    sets["X"] = Xa
    with np.errstate(all="ignore"):
        sets["Rt"] = Xa.astype(np.float32)
    sets["status"], sets["state"], sets["degenerate"] = init_status, state, degenerate
    res = np.zeros(P, PAIR_DTYPE)
    res["status"], res["used"] = status, usable
    res["cost"], res["w2"], res["v2"] = err
    summary = np.zeros(1, SUMMARY_DTYPE)
    s = summary[0]
    s["outer"], s["stop"], s["inner_total"], s["inner_last"] = K, stop, sum(inner[1:J + 1]), inner[J] if J else 0
    s["free_sets"], s["used_pairs"], s["held_last"] = free.sum(), usable.sum(), helds[J] if J else 0
    s["cost0"], s["cost"], s["rz0"] = costs[0], costs[K], rz0s[J] if J else 0.0
    return sets, res, summary[0]


# ---- the input families ---------------------------------------------------------------------------------------------------------------
NOISE_RAD, NOISE_TRANS = 0.01, 0.02
TOL = 1e-6  # the tolerances (radians, length units) the families are used with unless a test says otherwise
CG_TOL = 1e-3


class Family:
    """a list with its pose records, its info matrices (None: the identity) and the parameters of the call"""

    def __init__(self, n_sets, pairs, rt, info=None, R=None, t=None, **params):
        self.n_sets, self.pairs, self.rt = n_sets, np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2), np.ascontiguousarray(rt, np.float32)
        self.info = None if info is None else np.ascontiguousarray(info, np.float64).reshape(len(self.pairs), 36)
        self.R, self.t = R, t
        self.params = dict(dict(rot_tol=TOL, trans_tol=TOL, cg_tol=CG_TOL, anchor=0, max_outer=8, max_inner=64, flags=0), **params)
        self.use = self.statuses = self.info_statuses = None
        self.init_X = self.init_status = None  # where a family brings its start; else sync_start


def point_info(rt, seed, n_points=100):
    """a synthetic information matrix per pair: sum over n_points points q = R p + t, p uniform in [-1, 1]^3, of J^T J with
    J = [-[q]x, I], the Jacobian of exp(delta) q at delta = 0 (rotation first)"""
    rng = np.random.default_rng(seed)
    rt = np.asarray(rt, np.float64)
    out = np.zeros((len(rt), 36))
    for p in range(len(rt)):
        R, t = rt[p, :9].reshape(3, 3), rt[p, 9:]
        q = rng.uniform(-1, 1, (n_points, 3)) @ R.T + t
        H = np.zeros((6, 6))
        for v in q:
            Jm = np.zeros((3, 6))
            Jm[:, :3] = -np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
            Jm[:, 3:] = np.eye(3)
            H += Jm.T @ Jm
        out[p] = ((H + H.T) / 2).ravel()
    return out


def sync_start(f, max_rounds=32, tol=1e-4):
    """(init_X, init_status) of a family: sc_pairs_sync's reference on its list, as the chain runs it"""
    if f.init_X is not None:
        return f.init_X, f.init_status
    r2, e2 = SR.thresholds(tol, tol)
    sets, _res, _s = SR.sync(f.n_sets, f.pairs, f.rt, r2, e2, anchor=f.params["anchor"], max_rounds=max_rounds, use=f.use, statuses=f.statuses)
    return sets["X"].copy(), sets["status"].copy()


def run(f, init=None, **over):
    """the reference on a family -> (sets, pairs, summary)"""
    q = dict(f.params, **over)
    X0, st0 = init if init is not None else sync_start(f)
    r2, e2, cg2 = thresholds(q["rot_tol"], q["trans_tol"], q["cg_tol"])
    return solve(f.n_sets, f.pairs, f.rt, X0, st0, r2, e2, cg2, anchor=q["anchor"], max_outer=q["max_outer"], max_inner=q["max_inner"], use=f.use,
                 info=f.info, info_statuses=f.info_statuses if q["flags"] & INFO_STATUS else None, statuses=f.statuses if q["flags"] & STATUS else None)


def _noisy(rt, seed, rad=NOISE_RAD, trans=NOISE_TRANS):
    return SR.noisy(rt, seed, deg=float(np.rad2deg(rad)), trans=trans)


@functools.lru_cache(maxsize=None)
def ring40(info=True):
    """sync_ref.ring40's list at the issue's noise: 40 sets, the pairs (i, i + 1 mod 40) and nothing else"""
    g = SR.ring40()
    rt = _noisy(CR.relative_poses(g.pairs, g.R, g.t), 4001)
    return Family(40, g.pairs, rt, point_info(rt, 4002) if info else None, g.R, g.t)


@functools.lru_cache(maxsize=None)
def k24(rad=NOISE_RAD, trans=NOISE_TRANS, info=True):
    """sync_ref.k24's list — 24 sets, all 276 pairs — at the issue's noise"""
    g = SR.k24(False)
    rt = _noisy(g.rt, 2401, rad, trans)
    return Family(24, g.pairs, rt, point_info(rt, 2402) if info else None, g.R, g.t)


@functools.lru_cache(maxsize=None)
def strip200():
    """an odometry strip of 200 sets, the pairs (i, i + 1), with 40 closures between random sets at least 10 apart"""
    rng = np.random.default_rng(200)
    pairs = [(i, i + 1) for i in range(199)]
    seen = set(pairs)
    while len(pairs) < 239:
        i, k = sorted(int(v) for v in rng.integers(0, 200, 2))
        if k - i >= 10 and (i, k) not in seen:
            seen.add((i, k)); pairs.append((k, i) if rng.integers(2) else (i, k))
    pairs = np.array(pairs)
    R, t = CR.absolute_poses(200, 201)
    rt = _noisy(CR.relative_poses(pairs, R, t), 202)
    return Family(200, pairs, rt, point_info(rt, 203), R, t)


@functools.lru_cache(maxsize=None)
def exact24(anchor=0):
    """sync_ref.exact24: quarter-turn rotations, integer translations, all 276 pairs; the start is the truth in integers.  Every xi,
    g and rz_0 is exactly 0: one step, nothing moves, cost 0.0"""
    g = SR.exact24(anchor)
    f = Family(24, g.pairs, g.rt, None, g.R, g.t, rot_tol=0.0, trans_tol=0.0, anchor=anchor)
    f.init_X = SR.integers(g, anchor).astype(np.float64)
    f.init_status = np.zeros(24, np.int32)
    return f


@functools.lru_cache(maxsize=None)
def hub(n):
    """sync_ref.hub at n sets, at the issue's noise: set 0's sorted list has n - 1 entries"""
    g = SR.hub(n)
    rt = _noisy(CR.relative_poses(g.pairs, g.R, g.t), 3000 + n)
    return Family(n, g.pairs, rt, None, g.R, g.t, max_outer=2, max_inner=8)


@functools.lru_cache(maxsize=None)
def lattice(n):
    """n sets on a ring with the chords (i, i + 7): every set has four pairs"""
    pairs = np.array([(i, (i + 1) % n) for i in range(n)] + [((i + 7) % n, i) for i in range(n)])
    R, t = CR.absolute_poses(n, 5000 + n)
    rt = _noisy(CR.relative_poses(pairs, R, t), 6000 + n)
    f = Family(n, pairs, rt, None, R, t, max_outer=2, max_inner=6)
    f.init_X, f.init_status = SR.truth(f), np.zeros(n, np.int32)  # (sync would need many rounds: the start is the noiseless truth)
    return f


def edges():
    """k24 with the edge inputs of the header planted; the anchor is set 3, whose start is not the identity"""
    g = k24()
    f = Family(24, g.pairs.copy(), g.rt.copy(), g.info.copy(), g.R, g.t, anchor=3, flags=STATUS | INFO_STATUS)
    X0, st0 = sync_start(g)
    M = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    for s in range(24):  # the whole start moved by one rigid motion: the anchor's X is not the identity
        Rs, ts = X0[s, :9].reshape(3, 3), X0[s, 9:]
        X0[s, :9], X0[s, 9:] = (M @ Rs).ravel(), M @ ts + np.array([1.0, 2.0, 3.0])
    st0 = st0.copy()
    st0[5] = SC_ENOHYP          # unknown by its status
    X0[7, 4] = np.nan           # unknown by a NaN
    f.init_X, f.init_status = X0, st0
    f.statuses = np.zeros(276, np.int32); f.info_statuses = np.zeros(276, np.int32); f.use = np.ones(276, np.uint32)
    f.rt[10, 3] = np.inf        # an invalid pose
    f.statuses[11] = SC_ENOHYP  # a pose with a status
    f.pairs[12] = (9, 9)        # a self pair
    f.pairs[13] = f.pairs[14]; f.rt[13] = f.rt[14]  # a repeated pair
    f.use[15] = 0               # switched off
    f.info[16, 7] = np.nan      # an info record with a NaN
    f.info_statuses[17] = SC_EINVAL  # and one with a status
    return f


def held():
    """set 4 hangs on the ring 0-1-2-3 by one pair whose info is all zero: it is free, and held in every step"""
    pairs = np.array([(0, 1), (1, 2), (2, 3), (3, 0), (4, 2)])
    R, t = CR.absolute_poses(5, 77)
    rt = _noisy(CR.relative_poses(pairs, R, t), 78)
    info = np.tile(np.eye(6).ravel(), (5, 1))
    info[4] = 0.0
    return Family(5, pairs, rt, info, R, t)


def floating():
    """k24 beside a second world of 6 sets (24 .. 29, all pairs) that no pair joins to the first: known through the start, free,
    solved up to its own gauge"""
    g = SR.two_components()
    rt = _noisy(CR.relative_poses(g.pairs, g.R, g.t), 3030)
    f = Family(30, g.pairs, rt, None, g.R, g.t)
    X0 = np.zeros((30, 12))
    for s in range(30):
        a = 0 if s < 24 else 24
        X0[s, :9] = (g.R[a].T @ g.R[s]).ravel()
        X0[s, 9:] = g.R[a].T @ (g.t[s] - g.t[a])
    f.init_X, f.init_status = X0, np.zeros(30, np.int32)
    return f


ROSE_RAD, ROSE_TRANS = 0.1, 0.3
