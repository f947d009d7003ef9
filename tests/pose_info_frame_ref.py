"""The semantics of sc_pose_info_frame (include/saccot.h), restated per pose in Python loops over numpy float64 scalars: the contract
of sc_pose_info_batch — tests/pose_info_ref.py's terms, canonical_sum and assemble, imported unchanged — plus what the frame form adds:
the selection (SC_POSE_INFO_SEL_*) ANDed into the inlier set, and a status that is read only with SC_POSE_INFO_STATUS.  The reference
of tests/test_gpu_pose_info_frame.py; every comparison against it is bit for bit.  Also the scenes those tests share, so that
tests/test_pose_info_frame_abi.py can check on the CPU that they are what they are used for.  `O` is oracle/oracle.py."""
import numpy as np

import pose_info_ref as PI

SC_OK, SC_EINVAL, SC_ENOHYP = PI.SC_OK, PI.SC_EINVAL, PI.SC_ENOHYP
RESULT_DTYPE = PI.RESULT_DTYPE
SEL_NONE, SEL_MASK, SEL_LABEL = 0, 1, 2
STATUS = 1  # SC_POSE_INFO_STATUS
TAU = 0.05
SIZES = (65, 129, 512, 6600)  # one chunk and a bit, two and a bit, the batch form's maximum, and 104 chunks: two rounds of the deal


def one(O, src, tgt, Rt, tau, part=None, status=None):
    """-> the record of one pose on the frame (src, tgt): Rt (12,); part (n,) bool, the correspondences that take part (None: all);
    status: the record's int32 at byte 48 if the call reads it (SC_POSE_INFO_STATUS), else None"""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    Rt = np.ascontiguousarray(Rt, np.float32)
    out = np.zeros((), RESULT_DTYPE)
    if status is not None and int(status) != SC_OK:  # passed through
        out["status"] = status
        return out
    if not np.isfinite(Rt).all():
        out["status"] = SC_EINVAL
        return out
    mask, x, e = PI.terms(O, src, tgt, Rt, tau)
    if part is not None:
        mask = mask & np.asarray(part, bool).astype(np.uint8)
    c = int(mask.sum())
    if c == 0:  # all zeros
        return out
    s = [PI.canonical_sum(x[:, r], mask) for r in range(3)]
    M = {(r, q): PI.canonical_sum(x[:, r] * x[:, q], mask) for r, q in PI.PAIRS_RS}
    res = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    out["info"], out["sse"], out["inliers"] = PI.assemble(s, M, c), PI.canonical_sum(res, mask), c
    return out


def frame(O, src, tgt, poses, tau, sel_mode=SEL_NONE, sel=None, label0=0, statuses=None):
    """poses (K, 12) -> records (K,): the call on the frame (src, tgt) with the selection of sel_mode"""
    poses = np.asarray(poses, np.float32).reshape(-1, 12)
    out = np.zeros(len(poses), RESULT_DTYPE)
    for k, Rt in enumerate(poses):
        part = None
        if sel_mode == SEL_MASK:
            part = np.asarray(sel) != 0
        elif sel_mode == SEL_LABEL:
            part = np.asarray(sel, np.int32) == np.int32(label0 + k)
        out[k] = one(O, src, tgt, Rt, tau, part, None if statuses is None else statuses[k])
    return out


# ---- the scenes the tests of sc_pose_info_frame share ------------------------------------------------------------------------
def kw_of(tau=TAU):
    return PI.kw_of(tau)


def scene(pkg, n):
    return pkg.synth.make_scene(n, .3, 1.0, TAU, 7100 + n)


def rt_of(R, t):
    return np.concatenate([np.asarray(R, np.float32).ravel(), np.asarray(t, np.float32).ravel()])


def far(Rt):
    """the pose translated far away: no correspondence of a unit-sized scene is within tau of it"""
    out = np.array(Rt, np.float32)
    out[9:] += np.float32(1000.0)
    return out


def motions(pkg):
    """two rigid motions in one frame of 1500 correspondences (24 chunks): 25 % follow motion 0, 15 % motion 1"""
    return pkg.synth.make_scene_motions(1500, [.25, .15], 1.0, TAU, 7300)


def crafted_hole():
    """n = 192, every second correspondence follows the pose exactly; the selection clears the whole middle chunk -> (src, tgt, Rt, sel)"""
    src, tgt, Rt = PI._crafted_one(192, list(range(0, 192, 2)), 21)
    sel = np.ones(192, np.uint8); sel[64:128] = 0
    return src, tgt, Rt, sel


def crafted_last():
    """n = 129, every second correspondence follows the pose exactly, index 128 — alone in the last, partial chunk — among them; the
    selection keeps index 128 only -> (src, tgt, Rt, sel)"""
    src, tgt, Rt = PI._crafted_one(129, list(range(0, 129, 2)), 22)
    sel = np.zeros(129, np.uint8); sel[128] = 7  # (any non-zero byte)
    return src, tgt, Rt, sel
