"""The semantics of sc_polish_poses (include/saccot.h), restated per pose on the references that exist and nothing else:
tests/polish_ref.py::iterate's loop with `O.mask(...) & part` fed to O.refine — the CPU restatement takes a mask as it is —, O.score
over the participating rows, plus the status, pass-through and stop rules of sc_polish_batch and the four selections.  The reference
of tests/test_gpu_polish_poses.py; every comparison against it is bit for bit.  Also the scenes those tests share, so that
tests/test_polish_poses_abi.py can check on the CPU that they are what they are used for.  `O` is oracle/oracle.py."""
import numpy as np

import polish_batch_ref as PB

SC_OK, SC_EINVAL, SC_ENOHYP = PB.SC_OK, PB.SC_EINVAL, PB.SC_ENOHYP
STOP_FIXED, STOP_DECLINED, STOP_MAX_ITER = PB.STOP_FIXED, PB.STOP_DECLINED, PB.STOP_MAX_ITER
RESULT_DTYPE = PB.RESULT_DTYPE  # sc_polish_batch_result
SEL_NONE, SEL_MASK, SEL_LABEL, SEL_ALIVE = 0, 1, 2, 3
STATUS = 1  # SC_POLISH_POSES_STATUS
TAU = 0.05
# one chunk and a bit, two and a bit, the batch form's maximum, and 116 chunks: 9 x 116 > 1024, the smallest round size at which
# pass 2's deal of one lane per (chunk, entry of H) needs a second round (9 x 114 chunks > 1024 lanes: n > 7232)
SIZES = (65, 129, 512, 7400)
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def part_of(n, k, sel_mode=SEL_NONE, sel=None, label0=0):
    """-> (n,) bool: the correspondences that take part for pose k.  label0 + k wraps in 32 bits and is compared as int32."""
    if sel_mode == SEL_NONE:
        return np.ones(n, bool)
    if sel_mode == SEL_MASK:
        return np.asarray(sel) != 0
    lab = np.asarray(sel, np.int32)
    want = np.array([(int(label0) + int(k)) & 0xFFFFFFFF], np.uint32).view(np.int32)[0]
    if sel_mode == SEL_LABEL:
        return lab == want
    assert sel_mode == SEL_ALIVE
    return (lab < np.int32(label0)) | (lab >= want)


def _score(O, src, tgt, rt, part, tau, score_mode):
    if not part.any():
        return 0
    return int(O.score(np.ascontiguousarray(src[part]), np.ascontiguousarray(tgt[part]), rt[None, :], tau, score_mode=score_mode)[0])


def one(O, src, tgt, Rt, tau, part=None, status=None, score_mode=0, max_iter=16):
    """-> (record, mask) of one pose on the frame (src, tgt): Rt (12,); part (n,) bool (None: all); status: the record's int32 at
    byte 48 if the call reads it (SC_POLISH_POSES_STATUS), else None"""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    n = src.shape[0]
    part = np.ones(n, bool) if part is None else np.asarray(part, bool)
    rt0 = np.ascontiguousarray(Rt, np.float32).reshape(12)
    out = np.zeros((), RESULT_DTYPE)
    out["Rt"], out["stop"] = IDENT, STOP_DECLINED
    if status is not None and int(status) != SC_OK:  # passed through
        out["status"] = status
        return out, np.zeros(n, np.uint8)
    if not np.isfinite(rt0).all():
        out["status"] = SC_EINVAL
        return out, np.zeros(n, np.uint8)
    # polish_ref.iterate, with the selection ANDed into every inlier set
    rt, iters, stop = rt0.copy(), 0, STOP_MAX_ITER
    for _ in range(max_iter):
        mask = O.mask(src, tgt, rt, tau) & part.astype(np.uint8)
        done, rt2 = O.refine(src, tgt, mask, rt)
        if not done:
            stop = STOP_DECLINED
            break
        if rt2.tobytes() == rt.tobytes():
            stop = STOP_FIXED
            break
        rt = rt2
        iters += 1
    out["status"], out["Rt"], out["iters"], out["stop"] = SC_OK, rt, iters, stop
    out["score0"] = _score(O, src, tgt, rt0, part, tau, score_mode)
    out["score"] = _score(O, src, tgt, rt, part, tau, score_mode)
    return out, (O.mask(src, tgt, rt, tau) & part.astype(np.uint8)).copy()


def poses(O, src, tgt, pose_rt, tau, sel_mode=SEL_NONE, sel=None, label0=0, statuses=None, score_mode=0, max_iter=16):
    """pose_rt (K, 12) -> (records (K,), masks (K, n)): the call on the frame (src, tgt) with the selection of sel_mode"""
    pose_rt = np.asarray(pose_rt, np.float32).reshape(-1, 12)
    n = len(src)
    out = np.zeros(len(pose_rt), RESULT_DTYPE)
    masks = np.zeros((len(pose_rt), n), np.uint8)
    for k, Rt in enumerate(pose_rt):
        out[k], masks[k] = one(O, src, tgt, Rt, tau, part_of(n, k, sel_mode, sel, label0), None if statuses is None else statuses[k],
                               score_mode, max_iter)
    return out, masks


# ---- the scenes the tests of sc_polish_poses share ---------------------------------------------------------------------------
def kw_of(tau=TAU, **kw):
    return dict(PB.kw_of(tau), **kw)


def scene(pkg, n):
    return pkg.synth.make_scene(n, .3, 1.0, TAU, 7500 + n)


def rt_of(R, t):
    return np.concatenate([np.asarray(R, np.float32).ravel(), np.asarray(t, np.float32).ravel()])


def far(Rt):
    """the pose translated far away: no correspondence of a unit-sized scene is within tau of it"""
    out = np.array(Rt, np.float32)
    out[9:] += np.float32(1000.0)
    return out


def motions(pkg):
    """-> (scene, label): two rigid motions in one frame of 1500 correspondences (24 chunks), 25 % follow motion 0, 15 % motion 1, and a
    CRAFTED label array: the scene's own (-1 outliers, 0 motion 0) but for motion 1's true correspondences, of which every third gets
    -1, every third 0 and the rest 1.  Pose 1 then sees three nested inlier sets that differ: LABEL (a third of its correspondences),
    ALIVE (two thirds: those labelled 1 or -1) and NONE (all of them)."""
    sc = pkg.synth.make_scene_motions(1500, [.25, .15], 1.0, TAU, 7300)
    label = sc.label.copy()
    own = np.flatnonzero(sc.label == 1)
    label[own[0::3]] = -1
    label[own[1::3]] = 0
    return sc, label
