"""The semantics of sc_assign_poses (include/saccot.h), restated on the CPU: the reference of tests/test_gpu_assign_frame.py and
tests/test_gpu_assign_batch.py; every comparison against it is bit for bit.

O.mask and O.score (oracle/oracle.py) serve where they suffice — a pose's inliers, a labelled set's score — but SC_ASSIGN_BEST compares
residuals, so it needs the residual's BITS, which the restatement does not hand out.  `fmaf` below is an exact numpy emulation of the
fp32 fused multiply-add: the product of two fp32 values is exact in fp64; its sum with the addend is taken by a two-sum, whose error
term says whether the fp64 sum is inexact and on which side the exact value lies; an inexact sum is moved to the neighbour with an odd
last bit (round to odd), and a value rounded to odd at 53 bits rounds to nearest at 24 bits exactly as the unrounded value would.  A
plain fp64 add followed by a cast rounds twice and is wrong in one case in about 2^29.  tests/test_assign_abi.py pins `resid2` to the
C restatement's inlier test bit for bit.  Also the scenes those tests share, so that the CPU test can check what they are used for."""
import functools

import numpy as np

import polish_poses_ref as PF

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
BEST, FIRST = 0, 1
SEL_NONE, SEL_MASK = 0, 1
STATUS = 1  # SC_ASSIGN_STATUS
TAU = PF.TAU
RESULT_DTYPE = np.dtype([("status", np.int32), ("count", np.uint32), ("score", np.uint64), ("reserved", np.uint32, 4)])  # sc_assign_result
NO_D2 = np.array([0x7F800000], np.uint32).view(np.float32)[0]
kw_of, scene, rt_of, far = PF.kw_of, PF.scene, PF.rt_of, PF.far


def tau2_of(tau):
    """tau^2 as the masks derive it (oracle/oracle.py): tau is an fp32 parameter, its square is rounded once"""
    return np.float32(np.float64(np.float32(tau)) * np.float64(np.float32(tau)))


def fmaf(a, b, c):
    """fp32 fma(a, b, c), correctly rounded, elementwise"""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                             # exact: 24 + 24 bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)       # two-sum: p + c == s + err exactly (finite values)
        s, err = np.broadcast_arrays(s, err)
        s = np.array(s)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0)
        bits = s.view(np.int64)
        even = (bits & 1) == 0
        away = (err > 0) == (s > 0)           # the exact value lies on the far side of s from zero
        bits[fix & even & away] += 1          # ... the odd neighbour on that side
        bits[fix & even & ~away] -= 1
        return s.astype(np.float32)


def resid2(Rt, src, tgt):
    """the canonical fp32 squared residual of (R, t) on every correspondence (sc_arith.hpp resid2; inlier() of the restatement):
    Rt (12,) -> (n,), or Rt (K, 12) -> (K, n)"""
    M = np.asarray(Rt, np.float32)
    if M.ndim == 2:  # a block of poses at a time: the temporaries stay small
        return np.concatenate([_resid2(M[lo: lo + 32, :, None], src, tgt) for lo in range(0, len(M), 32)]) if len(M) else np.zeros((0, len(src)), np.float32)
    return _resid2(M.reshape(12), src, tgt)


def _resid2(M, src, tgt):
    M = np.moveaxis(M, -2 if M.ndim == 3 else 0, 0)  # M[c]: a scalar, or a (K, 1) column that broadcasts against the (n,) rows
    p, q = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    with np.errstate(all="ignore"):
        e = [M[9 + r] + fmaf(M[3 * r + 2], p[:, 2], fmaf(M[3 * r + 1], p[:, 1], fmaf(M[3 * r], p[:, 0], -q[:, r]))) for r in range(3)]
        return fmaf(e[2], e[2], fmaf(e[1], e[1], e[0] * e[0]))


def assign(O, src, tgt, poses, tau, mode=BEST, part=None, statuses=None, score_mode=0):
    """poses (K, 12); part (n,) bool or None; statuses: the int32 at byte 48 of every record if the call reads it, else None
    -> (label (n,) int32, d2 (n,) float32, records (K,))"""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    poses = np.asarray(poses, np.float32).reshape(-1, 12)
    n, K = len(src), len(poses)
    part = np.ones(n, bool) if part is None else np.asarray(part) != 0
    tau2 = tau2_of(tau)
    out = np.zeros(K, RESULT_DTYPE)
    label = np.full(n, -1, np.int32)
    d2 = np.full(n, NO_D2, np.float32)
    if statuses is not None:
        out["status"] = statuses  # passed through
    out["status"][(out["status"] == SC_OK) & ~np.isfinite(poses).all(axis=1)] = SC_EINVAL
    valid = np.flatnonzero(out["status"] == SC_OK)
    D = resid2(poses[valid], src, tgt)
    for row, k in enumerate(valid):
        d = D[row]
        with np.errstate(invalid="ignore"):
            cand = part & (d < tau2)
            take = cand & ((d < d2) if mode == BEST else (label < 0))  # a strictly smaller residual: ties stay with the lowest k
        label[take], d2[take] = k, d[take]
    count = np.bincount(label[label >= 0], minlength=K)
    out["count"] = count
    for k in np.flatnonzero(count):
        idx = np.flatnonzero(label == k)
        out[k]["score"] = len(idx) if score_mode == 0 else int(
            O.score(np.ascontiguousarray(src[idx]), np.ascontiguousarray(tgt[idx]), poses[k][None, :], tau, score_mode=score_mode)[0])
    return label, d2, out


def batch(O, problems, poses, tau, mode=BEST, statuses=None, score_mode=0):
    """problems: list of (src, tgt); poses (K, B, 12) motion-major; statuses (K, B) -> (list of labels, records (K, B))"""
    poses = np.asarray(poses, np.float32)
    K, B = poses.shape[:2]
    out = np.zeros((K, B), RESULT_DTYPE)
    labels = []
    for b, (s, t) in enumerate(problems):
        if not (np.isfinite(s).all() and np.isfinite(t).all()):
            out[:, b]["status"] = SC_EINVAL
            labels.append(np.full(len(s), -1, np.int32))
            continue
        lab, _, out[:, b] = assign(O, s, t, poses[:, b], tau, mode, None, None if statuses is None else statuses[:, b], score_mode)
        labels.append(lab)
    return labels, out


# ---- the scenes and pose lists the tests of sc_assign_poses share ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def motions(pkg):
    """two rigid motions in one frame of 1500 correspondences: 25 % follow motion 0, 15 % motion 1"""
    return pkg.synth.make_scene_motions(1500, [.25, .15], 1.0, TAU, 7300)


def perturbed(Rt, k, seed, angle=2e-3, shift=4e-3):
    """k polished-looking neighbours of the pose Rt: a small seeded rotation (about `angle` radians) and translation (about `shift`,
    a fraction of tau) composed on the left — poses whose inlier sets overlap, so BEST has something to decide"""
    rng = np.random.default_rng(seed)
    R, t = np.asarray(Rt[:9], np.float64).reshape(3, 3), np.asarray(Rt[9:], np.float64)
    out = np.zeros((k, 12), np.float32)
    for i in range(k):
        w = rng.normal(size=3) * angle
        th = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        dR = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th**2 * (Kx @ Kx)
        out[i] = rt_of(dR @ R, dR @ t + rng.normal(size=3) * shift)
    return out


def many(Rt, K, seed):
    """K poses for the large pose counts: neighbours of Rt, every seventh a pose far away (it claims nothing), and one exact copy of
    an earlier pose (under BEST a copy never wins a tie against its original)"""
    out = perturbed(Rt, K, seed)
    out[3::7] = far(Rt)
    if K > 5:
        out[5] = out[1]
    return out


def hostile():
    """a finite pose with entries near FLT_MAX: its residual is inf or NaN on any ordinary correspondence"""
    big = np.float32(3e38)
    return np.array([big, -big, big, -big, big, -big, big, -big, big, big, -big, big], np.float32)
