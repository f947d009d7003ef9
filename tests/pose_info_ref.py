"""The semantics of sc_pose_info_batch (include/saccot.h), restated per problem in Python loops over numpy float64 scalars, in
exactly the order the contract gives: the inlier set is O.mask's, x = R p + t and the residual are formed in fp64 with the contract's
parentheses, the ten sums run over chunks of 64 consecutive indices sequentially from 0.0 and then over the chunk sums, and the
matrix is assembled entry by entry.  The reference of tests/test_gpu_pose_info.py; every comparison against it is bit for bit.
Slot and pairs expansion reuse match_batch_ref.py / pairs_ref.py.  Also the scenes those tests share, so that
tests/test_pose_info_abi.py can check on the CPU that they are what they are used for.  `O` is oracle/oracle.py."""
import numpy as np

import batch_ref
import polish_batch_ref as PB

SC_OK, SC_EINVAL, SC_ENOHYP = batch_ref.SC_OK, batch_ref.SC_EINVAL, batch_ref.SC_ENOHYP
RESULT_DTYPE = np.dtype([("info", np.float64, 36), ("sse", np.float64), ("status", np.int32), ("inliers", np.uint32),
                         ("reserved", np.uint32, 4)])  # sc_pose_info_result
CHUNK = 64
PAIRS_RS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # the order of m_rs
TAUS = (0.05, 0.02)
F64 = np.float64


def terms(O, src, tgt, Rt, tau):
    """-> (mask (n,) uint8, x (n, 3) float64, e (n, 3) float64) of finite inputs: the canonical inlier test and the fp64 terms"""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    Rt = np.ascontiguousarray(Rt, np.float32)
    n = src.shape[0]
    mask = O.mask(src, tgt, Rt, tau).copy()
    x = np.zeros((n, 3), F64); e = np.zeros((n, 3), F64)
    for m in range(n):
        p0, p1, p2 = F64(src[m, 0]), F64(src[m, 1]), F64(src[m, 2])
        for r in range(3):
            x[m, r] = ((F64(Rt[3 * r]) * p0 + F64(Rt[3 * r + 1]) * p1) + F64(Rt[3 * r + 2]) * p2) + F64(Rt[9 + r])
            e[m, r] = x[m, r] - F64(tgt[m, r])
    return mask, x, e


def canonical_sum(values, mask):
    """the library's canonical order: chunks of 64 consecutive indices, sequentially from 0.0 over the chunk's inliers, then the
    chunk sums sequentially in chunk order"""
    total = F64(0.0)
    for lo in range(0, len(values), CHUNK):
        c = F64(0.0)
        for m in range(lo, min(lo + CHUNK, len(values))):
            if mask[m]:
                c = c + values[m]
        total = total + c
    return total


def assemble(s, M, c):
    """info (36,) from s (3,), M: {(r, s): m_rs for r <= s}, the count c — the contract's assembly, entry by entry"""
    info = np.zeros((6, 6), F64)
    info[0, 0] = M[1, 1] + M[2, 2]; info[1, 1] = M[0, 0] + M[2, 2]; info[2, 2] = M[0, 0] + M[1, 1]
    for r, q in ((0, 1), (0, 2), (1, 2)):
        info[r, q] = info[q, r] = -M[r, q]
    sx = ((F64(0.0), -s[2], s[1]), (s[2], F64(0.0), -s[0]), (-s[1], s[0], F64(0.0)))
    for r in range(3):
        for k in range(3):
            info[r, 3 + k] = sx[r][k]
            info[3 + k, r] = sx[r][k]
        info[3 + r, 3 + r] = F64(c)
    return info.reshape(36)


def one(O, src, tgt, rec_status, Rt, tau):
    """-> the record of one problem: src, tgt (n, 3); rec_status and Rt (12,): its input pose record"""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    Rt = np.ascontiguousarray(Rt, np.float32)
    out = np.zeros((), RESULT_DTYPE)
    if int(rec_status) != SC_OK:  # passed through
        out["status"] = rec_status
        return out
    if not (np.isfinite(src).all() and np.isfinite(tgt).all() and np.isfinite(Rt).all()):
        out["status"] = SC_EINVAL
        return out
    mask, x, e = terms(O, src, tgt, Rt, tau)
    c = int(mask.sum())
    if c == 0:  # all zeros
        return out
    s = [canonical_sum(x[:, r], mask) for r in range(3)]
    M = {(r, q): canonical_sum(x[:, r] * x[:, q], mask) for r, q in PAIRS_RS}  # (elementwise fp64 products, rounded once each)
    res = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    out["info"], out["sse"], out["inliers"] = assemble(s, M, c), canonical_sum(res, mask), c
    return out


def batch(O, problems, poses, tau):
    """problems: list of (src, tgt); poses: their input records (any dtype with Rt and status) -> records (B,)"""
    out = np.zeros(len(problems), RESULT_DTYPE)
    for b, (s, t) in enumerate(problems):
        out[b] = one(O, s, t, poses[b]["status"], poses[b]["Rt"], tau)
    return out


def slots_one(O, src_pts, tgt_pts, corr, n, flag, rec_status, Rt, tau):
    """one problem of the slot form: its points, the first n entries of its slot (indices local to the problem), its count pair"""
    out = np.zeros((), RESULT_DTYPE)
    cap_bad = n > len(corr)
    if flag or n < 3 or cap_bad:
        out["status"] = rec_status if int(rec_status) != SC_OK else SC_EINVAL
        return out
    if int(rec_status) != SC_OK:
        out["status"] = rec_status
        return out
    corr = np.asarray(corr[:n], np.int64)
    if (corr[:, 0] < 0).any() or (corr[:, 0] >= len(src_pts)).any() or (corr[:, 1] < 0).any() or (corr[:, 1] >= len(tgt_pts)).any():
        out["status"] = SC_EINVAL
        return out
    return one(O, np.asarray(src_pts, np.float32)[corr[:, 0]], np.asarray(tgt_pts, np.float32)[corr[:, 1]], rec_status, Rt, tau)


# ---- the scenes the tests of sc_pose_info_batch share ------------------------------------------------------------------------
def kw_of(tau):
    return PB.kw_of(tau)


def mixed(pkg):
    """polish_batch_ref.mixed: n = 3, 4, 63, 64, 65, 128, 129, 257, 512, 512"""
    return PB.mixed(pkg)


def _pose(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    R = q * np.sign(np.linalg.det(q))
    return np.concatenate([R.ravel(), rng.uniform(-1, 1, size=3)]).astype(np.float32)


def _crafted_one(n, inliers, seed):
    """n correspondences under a ground-truth pose; those not listed in `inliers` are moved 10 units away"""
    rng = np.random.default_rng(seed)
    Rt = _pose(seed + 1)
    src = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    tgt = src.astype(np.float64) @ Rt[:9].astype(np.float64).reshape(3, 3).T + Rt[9:].astype(np.float64)
    out = np.ones(n, bool); out[list(inliers)] = False
    tgt[out] += 10.0
    return src, tgt.astype(np.float32), Rt


FLT_BIG = np.float32(3.0e38)  # within 12 % of FLT_MAX


def crafted():
    """-> (names, problems [(src, tgt)], poses (B,) of batch_ref.RESULT_DTYPE with status SC_OK and the ground-truth Rt):
    last     n = 129, the only inlier is index 128: every inlier in the last chunk, which holds one correspondence
    hole     n = 192, chunks 0 and 2 hold inliers, the middle chunk none
    none     n = 64, no inlier
    two      n = 65, two inliers, one either side of the chunk end
    huge     n = 70, identity pose, p == q, coordinates up to +-3e38: every correspondence an inlier, products near FLT_MAX^2"""
    names = ("last", "hole", "none", "two", "huge")
    made = [_crafted_one(129, [128], 11), _crafted_one(192, list(range(0, 64, 3)) + list(range(130, 192, 2)), 12),
            _crafted_one(64, [], 13), _crafted_one(65, [63, 64], 14)]
    rng = np.random.default_rng(15)
    big = (rng.uniform(-1, 1, size=(70, 3)) * np.float64(FLT_BIG)).astype(np.float32)
    big[0] = (FLT_BIG, -FLT_BIG, FLT_BIG)
    made.append((big, big.copy(), batch_ref.IDENT.copy()))
    poses = np.zeros(len(made), batch_ref.RESULT_DTYPE)
    for b, (_, _, Rt) in enumerate(made):
        poses[b]["Rt"], poses[b]["status"] = Rt, SC_OK
    return names, [(s, t) for s, t, _ in made], poses
