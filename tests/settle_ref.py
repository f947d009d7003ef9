"""The semantics of sc_settle_poses (include/saccot.h), restated on the CPU from the two references that exist and nothing else:
rounds of tests/assign_ref.py::assign (BEST) followed by tests/polish_poses_ref.py::poses (SEL_LABEL, max_iter = 1), with the
stopping and record rules of the header.  The reference of tests/test_gpu_settle_frame.py and tests/test_gpu_settle_batch.py; every
comparison against it is bit for bit.  Also the scenes and pose lists those tests share, so that tests/test_settle_abi.py can check
on the CPU that they are what they are used for.  `O` is oracle/oracle.py."""
import functools

import numpy as np

import assign_ref as AR
import polish_poses_ref as PF

SC_OK, SC_EINVAL, SC_ENOHYP = AR.SC_OK, AR.SC_EINVAL, AR.SC_ENOHYP
STOP_FIXED, STOP_DECLINED, STOP_MAX_ITER = PF.STOP_FIXED, PF.STOP_DECLINED, PF.STOP_MAX_ITER
RESULT_DTYPE = PF.RESULT_DTYPE  # sc_polish_batch_result
SEL_NONE, SEL_MASK = AR.SEL_NONE, AR.SEL_MASK
STATUS = 1  # SC_SETTLE_STATUS
TAU = AR.TAU
IDENT = PF.IDENT


def _invalid_record(status):
    out = np.zeros((), RESULT_DTYPE)
    out["Rt"], out["status"], out["stop"] = IDENT, status, STOP_DECLINED
    return out


def settle(O, src, tgt, poses, tau, part=None, statuses=None, score_mode=0, max_iter=16):
    """poses (K, 12); part (n,) bool or None; statuses: the int32 at byte 48 of every record if the call reads it, else None
    -> (records (K,), label (n,) int32, d2 (n,) float32, rounds (2,) uint32: counted rounds, the call's stop)"""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    P = np.array(poses, np.float32).reshape(-1, 12)
    K = len(P)
    st = np.zeros(K, np.int32) if statuses is None else np.array(statuses, np.int32)
    st[(st == SC_OK) & ~np.isfinite(P).all(axis=1)] = SC_EINVAL  # invalid in P_0: invalid for good
    valid = st == SC_OK
    iters = np.zeros(K, np.int64)
    declined = np.ones(K, bool)
    rounds, stop, score0 = 0, STOP_MAX_ITER, None
    final = None
    for _ in range(max_iter):
        lab, d2, asg = AR.assign(O, src, tgt, P, tau, AR.BEST, part, st, score_mode)
        if score0 is None:
            score0 = asg["score"].copy()
        pol = PF.poses(O, src, tgt, P, tau, PF.SEL_LABEL, lab, 0, statuses=st, score_mode=score_mode, max_iter=1)[0]
        declined = pol["stop"] == STOP_DECLINED
        changed = np.array([valid[k] and pol["Rt"][k].tobytes() != P[k].tobytes() for k in range(K)], bool)
        if not changed.any():
            stop, final = STOP_FIXED, (lab, d2, asg)  # this round is not counted; its labels are the labels under the final poses
            break
        iters += changed
        P[valid] = pol["Rt"][valid]
        rounds += 1
    if final is None:
        final = AR.assign(O, src, tgt, P, tau, AR.BEST, part, st, score_mode)
    lab, d2, asg = final
    out = np.zeros(K, RESULT_DTYPE)
    for k in range(K):
        if not valid[k]:
            out[k] = _invalid_record(st[k])
            continue
        out[k]["Rt"], out[k]["status"] = P[k], SC_OK
        out[k]["score0"], out[k]["score"] = int(score0[k]) & 0xFFFFFFFF, int(asg["score"][k]) & 0xFFFFFFFF
        out[k]["iters"], out[k]["stop"] = iters[k], STOP_DECLINED if declined[k] else stop
    return out, lab, d2, np.array([rounds, stop], np.uint32)


def composed(O, src, tgt, poses, tau, rounds, part=None, statuses=None, score_mode=0):
    """equality 1 on the references: `rounds` rounds of assign(BEST) + poses(SEL_LABEL, max_iter 1), each fed the round before's
    records, and a last assign -> (Rt (K, 12), label, d2, assign records)"""
    pol = np.zeros(len(poses), RESULT_DTYPE)
    pol["Rt"], pol["status"] = poses, 0 if statuses is None else statuses
    read = statuses is not None
    for _ in range(rounds):
        lab = AR.assign(O, src, tgt, pol["Rt"], tau, AR.BEST, part, pol["status"] if read else None, score_mode)[0]
        pol = PF.poses(O, src, tgt, pol["Rt"], tau, PF.SEL_LABEL, lab, 0, statuses=pol["status"] if read else None, score_mode=score_mode,
                       max_iter=1)[0]
        read = True  # the records carry a status from here on
    return (pol["Rt"],) + AR.assign(O, src, tgt, pol["Rt"], tau, AR.BEST, part, pol["status"] if read else None, score_mode)


def batch(O, problems, poses, tau, statuses=None, score_mode=0, max_iter=16):
    """problems: list of (src, tgt); poses (K, B, 12) motion-major; statuses (K, B) (always read)
    -> (records (K, B), list of labels, rounds (B, 2))"""
    poses = np.asarray(poses, np.float32)
    K, B = poses.shape[:2]
    out = np.zeros((K, B), RESULT_DTYPE)
    rounds = np.zeros((B, 2), np.uint32)
    labels = []
    for b, (s, t) in enumerate(problems):
        if not (np.isfinite(s).all() and np.isfinite(t).all()):
            out[:, b] = _invalid_record(SC_EINVAL)
            rounds[b] = 0, STOP_DECLINED
            labels.append(np.full(len(s), -1, np.int32))
            continue
        st = np.zeros(K, np.int32) if statuses is None else statuses[:, b]
        out[:, b], lab, _, rounds[b] = settle(O, s, t, poses[:, b], tau, None, st, score_mode, max_iter)
        labels.append(lab)
    return out, labels, rounds


# ---- the scenes and pose lists the tests of sc_settle_poses share ------------------------------------------------------------------
kw_of, scene, rt_of, far, motions, perturbed, many = AR.kw_of, AR.scene, AR.rt_of, AR.far, AR.motions, AR.perturbed, AR.many


@functools.lru_cache(maxsize=None)
def starts(pkg):
    """the pose lists on the two-motion scene AR.motions (n = 1500), by name: what each is used for is checked by
    tests/test_settle_abi.py on this reference"""
    mo = motions(pkg)
    gt = [rt_of(R, t) for R, t in mo.motions]
    pert = np.stack([perturbed(gt[0], 1, 11, 1e-2, 2e-2)[0], perturbed(gt[1], 1, 12, 1e-2, 2e-2)[0]])
    return {
        "gt": np.stack(gt),                                                # settles at once
        "perturbed": pert,                                                 # one start per motion: a few rounds to the fixed point
        "far_dup": np.stack([pert[0], pert[1], far(gt[0]), pert[0]]),      # K = 4: a pose that claims nothing, a copy that loses every tie
        "many8": np.concatenate([many(gt[0], 5, 3), many(gt[1], 3, 4)]),   # K = 8: neighbours that trade correspondences for long
        "many64": np.concatenate([many(gt[0], 40, 5), many(gt[1], 24, 6)]),  # K = 64: most poses starve
    }
