"""The semantics of sc_merge_poses (include/saccot.h), restated on the CPU: the reference of tests/test_gpu_merge_frame.py and
tests/test_gpu_merge_batch.py; every comparison against it is bit for bit.

The support sets come from tests/assign_ref.py::resid2, which carries the BITS of the canonical residual, compared with tau^2 as the
masks derive it; a pose's score is O.score (oracle/oracle.py) over its own inlier rows; everything after that is integers.  Also the
pose lists those tests share, so that tests/test_merge_abi.py can check on the CPU that they are what they are used for."""
import functools

import numpy as np

import assign_ref as AR

SC_OK, SC_EINVAL, SC_ENOHYP = AR.SC_OK, AR.SC_EINVAL, AR.SC_ENOHYP
OVER_MIN, OVER_UNION = 0, 1
SEL_NONE, SEL_MASK = AR.SEL_NONE, AR.SEL_MASK
STATUS, COMPACT = 1, 2  # SC_MERGE_STATUS, SC_MERGE_COMPACT
TAU = AR.TAU
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
POSE_DTYPE = np.dtype([("Rt", np.float32, 12), ("status", np.int32), ("index", np.int32), ("count", np.uint32), ("score", np.uint32)])  # sc_merge_pose
kw_of, scene, rt_of, far, motions, perturbed, many, hostile = AR.kw_of, AR.scene, AR.rt_of, AR.far, AR.motions, AR.perturbed, AR.many, AR.hostile


def support(O, src, tgt, poses, tau, part=None, statuses=None, score_mode=0):
    """-> (status (K,) int32, I (K, n) bool: pose k's own inlier set, count (K,), score (K,)): an invalid pose has an empty set"""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    P = np.asarray(poses, np.float32).reshape(-1, 12)
    n, K = len(src), len(P)
    part = np.ones(n, bool) if part is None else np.asarray(part) != 0
    st = np.zeros(K, np.int32) if statuses is None else np.array(statuses, np.int32)
    st[(st == SC_OK) & ~np.isfinite(P).all(axis=1)] = SC_EINVAL
    valid = np.flatnonzero(st == SC_OK)
    inl = np.zeros((K, n), bool)
    with np.errstate(invalid="ignore"):
        inl[valid] = part[None, :] & (AR.resid2(P[valid], src, tgt) < AR.tau2_of(tau))  # a float '<': a NaN residual is no candidate
    count = inl.sum(axis=1).astype(np.int64)
    score = count.copy()
    if score_mode != 0:
        for k in np.flatnonzero(count):
            idx = np.flatnonzero(inl[k])
            score[k] = int(O.score(np.ascontiguousarray(src[idx]), np.ascontiguousarray(tgt[idx]), P[k][None, :], tau, score_mode=score_mode)[0])
    return st, inl, count, score & 0xFFFFFFFF


def same(x, cj, ck, measure, num, den):
    """integers only (Python's: no width to overflow)"""
    base = (cj + ck - x) if measure == OVER_UNION else min(cj, ck)
    return x >= 1 and x * den >= num * base


def strength_order(score):
    """larger score first, ties to the lower k"""
    return sorted(range(len(score)), key=lambda k: (-int(score[k]), k))


def merge(O, src, tgt, poses, tau, part=None, statuses=None, score_mode=0, measure=OVER_MIN, num=1, den=2, min_count=0, compact=False):
    """poses (K, 12); part (n,) or None; statuses: the int32 at byte 48 of every record if the call reads it, else None
    -> (records (K,) of POSE_DTYPE, parent (K,) int32, overlap (K, K) uint32, count (2,) uint32: the kept poses, the valid poses)"""
    P = np.asarray(poses, np.float32).reshape(-1, 12)
    K = len(P)
    st, inl, cnt, score = support(O, src, tgt, P, tau, part, statuses, score_mode)
    bits = inl.astype(np.int64)
    x = bits @ bits.T
    parent = np.full(K, -1, np.int32)
    kept = []  # in strength order
    for k in strength_order(score):
        if st[k] != SC_OK or cnt[k] < min_count:
            continue
        into = next((j for j in kept if same(int(x[j, k]), int(cnt[j]), int(cnt[k]), measure, num, den)), None)
        if into is None:
            kept.append(k)
            parent[k] = k
        else:
            parent[k] = into
    rec = np.zeros(K, POSE_DTYPE)
    rec["Rt"], rec["index"] = IDENT, parent
    for k in range(K):
        if parent[k] == k:
            rec[k]["Rt"], rec[k]["status"] = P[k], SC_OK
        else:
            rec[k]["status"] = SC_ENOHYP if st[k] == SC_OK else st[k]
        if st[k] == SC_OK:
            rec[k]["count"], rec[k]["score"] = cnt[k], score[k]
    if compact:
        is_kept = parent == np.arange(K)
        rec = np.concatenate([rec[is_kept], rec[~is_kept]])
    return rec, parent, x.astype(np.uint32), np.array([len(kept), int((st == SC_OK).sum())], np.uint32)


def batch(O, problems, poses, tau, statuses=None, score_mode=0, **rule):
    """problems: list of (src, tgt); poses (K, B, 12) motion-major; statuses (K, B) (always read)
    -> (records (K, B), parent (K, B), count (B, 2)): the frame reference per problem"""
    poses = np.asarray(poses, np.float32)
    K, B = poses.shape[:2]
    out = np.zeros((K, B), POSE_DTYPE)
    parent = np.full((K, B), -1, np.int32)
    count = np.zeros((B, 2), np.uint32)
    for b, (s, t) in enumerate(problems):
        if not (np.isfinite(s).all() and np.isfinite(t).all()):
            out[:, b]["Rt"], out[:, b]["status"], out[:, b]["index"] = IDENT, SC_EINVAL, -1
            continue
        st = np.zeros(K, np.int32) if statuses is None else statuses[:, b]
        out[:, b], parent[:, b], _, count[b] = merge(O, s, t, poses[:, b], tau, None, st, score_mode, **rule)
    return out, parent, count


# ---- the pose lists the tests of sc_merge_poses share, on the two-motion scene AR.motions (n = 1500) -----------------------------------
NEAR_ANGLE, NEAR_SHIFT = 8e-3, 2e-2  # the perturbation of `near`: tests/test_merge_abi.py holds the condition these sizes meet


def _contained(mo, Rt):
    """the pose Rt pushed about tau away along one axis: the first push (a fixed order of candidates) whose support is at
    least 3 correspondences, fewer than Rt's, and lies INSIDE Rt's — exactly, so that num == den folds it"""
    tau2 = AR.tau2_of(TAU)
    whole = AR.resid2(Rt, mo.src, mo.tgt) < tau2
    for frac in (0.8, 1.0, 1.2, 1.3, 1.4, 1.5):
        for axis in range(3):
            for sign in (1.0, -1.0):
                out = Rt.copy()
                out[9 + axis] += np.float32(sign * frac * TAU)
                own = AR.resid2(out, mo.src, mo.tgt) < tau2
                if 3 <= own.sum() < whole.sum() and not (own & ~whole).any():
                    return out
    raise AssertionError("no candidate's support lies inside the pose's")


@functools.lru_cache(maxsize=None)
def lists(pkg):
    """by name; what each is used for is checked by tests/test_merge_abi.py on this reference"""
    mo = motions(pkg)
    gt = [rt_of(R, t) for R, t in mo.motions]
    dup = many(gt[0], 8, 21)                # neighbours of motion 0; [3] far away; [5] an exact copy of [1]
    dup[0] = perturbed(gt[0], 1, 22, 1.5e-2, 3e-2)[0]  # a weak copy of motion 0 numbered BELOW the strong ones: it folds by strength
    dup[6], dup[7] = gt[0], gt[1]
    near = np.concatenate([perturbed(gt[0], 5, 31, NEAR_ANGLE, NEAR_SHIFT), perturbed(gt[1], 3, 32, NEAR_ANGLE, NEAR_SHIFT)])
    nested = np.stack([_contained(mo, gt[0]), gt[1], gt[0]])
    bad = gt[0].copy()
    bad[4] = np.nan
    invalid = np.stack([gt[0], bad, hostile(), far(gt[0]), gt[1], gt[0]])  # a NaN pose, a NaN residual, an empty support, a copy
    starved = np.concatenate([gt, perturbed(gt[0], 6, 41, 3e-2, 6e-2)])   # K = 8: most poses hold a handful of inliers
    return {"dup": dup, "near": near, "nested": nested, "invalid": invalid, "starved": starved,
            "many64": np.concatenate([many(gt[0], 40, 5), many(gt[1], 24, 6)])}
