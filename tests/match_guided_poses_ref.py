"""The semantics of sc_match_guided_poses (include/saccot.h), restated in numpy: the reference of
tests/test_gpu_match_guided_poses.py; every comparison against it is bit for bit.  Nothing of the single-pose restatement is
changed: the gate residual of record k is match_guided_ref.gate_residuals, its admissibility match_guided_ref.admissible, and the
union — the OR over the USED records — goes through match_guided_ref.select.  label / g2 of a pair are a stable arg-min over the
used records with NaN set to +inf (an unused record: +inf too).  Also the scenes the tests share, so that the CPU test can check what
they are used for."""
import numpy as np

import assign_ref as AR
import match_guided_ref as MG
import match_ref

SC_OK = 0
GATE = MG.GATE
RECORD_DTYPE = np.dtype([("Rt", np.float32, 12), ("status", np.int32), ("pad", np.uint32, 7)])  # 80 bytes: sc_batch_result's size
assert RECORD_DTYPE.itemsize == 80


def records(poses, status=None):
    """(K, 12) poses -> K records of 80 bytes with a status at byte 48 (all SC_OK unless given)"""
    poses = np.asarray(poses, np.float32).reshape(-1, 12)
    rec = np.zeros(len(poses), RECORD_DTYPE)
    rec["Rt"] = poses
    rec["pad"] = 0xDEADBEEF  # nothing behind the status is the library's business
    if status is not None:
        rec["status"] = status
    return rec


class Problem:
    """one (scene, pose list, gate): the distances, the residuals, the union mask and the labels, shared by the modes"""

    def __init__(self, src_pts, fsrc, tgt_pts, ftgt, poses, gate, used=None):
        poses = np.asarray(poses, np.float32).reshape(-1, 12)
        K = len(poses)
        used = np.ones(K, bool) if used is None else np.asarray(used, bool)
        self.acc = match_ref.distances(fsrc, ftgt)
        ns, nt = self.acc.shape
        self.adm = np.zeros((ns, nt), bool)
        self.adm_k = np.zeros((K, ns, nt), bool)  # per record, for what the tests say about the scenes
        g = np.full((K, ns, nt), np.inf, np.float32)
        for k in range(K):
            if not used[k]:
                continue  # a record that is not used is neither read for the gate nor looked at otherwise
            gk = MG.gate_residuals(poses[k], src_pts, tgt_pts)
            self.adm_k[k] = MG.admissible(gk, gate)
            self.adm |= self.adm_k[k]
            g[k] = np.where(np.isnan(gk), np.float32(np.inf), gk)
        self.label = np.argmin(g, axis=0).astype(np.int32)  # (the first of equal minima: the lowest k)
        self.g2 = np.take_along_axis(g, self.label[None].astype(np.int64), axis=0)[0]

    def match(self, **kw):
        """-> (corr (n, 2) int32, d2 (n,), g2 (n,), label (n,) int32) in ascending (source row, rank) order"""
        corr, d2, g2 = MG.select(self.acc, self.g2, self.adm, **kw)
        return corr, d2, g2, self.label[corr[:, 0], corr[:, 1]].astype(np.int32)


def match(src_pts, fsrc, tgt_pts, ftgt, poses, gate, used=None, **kw):
    return Problem(src_pts, fsrc, tgt_pts, ftgt, poses, gate, used).match(**kw)


# ---- the scenes the tests share ----------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, src_pts, fsrc, tgt_pts, ftgt, poses):
        self.src_pts, self.fsrc, self.tgt_pts, self.ftgt, self.poses = src_pts, fsrc, tgt_pts, ftgt, np.asarray(poses, np.float32).reshape(-1, 12)

    def args(self):
        return self.src_pts, self.fsrc, self.tgt_pts, self.ftgt, self.poses

    def with_poses(self, poses):
        return Scene(self.src_pts, self.fsrc, self.tgt_pts, self.ftgt, poses)


def scene(seed, ns, nt, D, K, sd=0.3, noise=0.01):
    """Source points fill the unit cube in K groups (row i belongs to group i % K); K random poses; the first nt // 2 target rows
    (at most ns) are copies of source rows, each planted under the pose of ITS group with small point noise and a noisy descriptor
    copy; the remaining target rows are clutter: random points of the cube under a random pose of the list, random descriptors."""
    rng = np.random.default_rng(seed)
    src = rng.random((ns, 3))
    Rs, ts = zip(*[MG.random_pose(rng) for _ in range(K)])
    fsrc = rng.standard_normal((ns, D)).astype(np.float32)
    ftgt = rng.standard_normal((nt, D)).astype(np.float32)
    which = rng.integers(0, K, nt)
    tgt = np.stack([rng.random(3) @ Rs[k].T + ts[k] for k in which])
    m = min(ns, nt // 2)
    if m:
        rows = rng.permutation(ns)[:m]
        for c, i in enumerate(rows):
            g = i % K
            tgt[c] = src[i] @ Rs[g].T + ts[g] + noise * rng.standard_normal(3)
        ftgt[:m] = fsrc[rows] + np.float32(sd) * rng.standard_normal((m, D)).astype(np.float32)
    return Scene(src.astype(np.float32), fsrc, tgt.astype(np.float32), ftgt, [AR.rt_of(R, t) for R, t in zip(Rs, ts)])


def shared_scene(ns, nt, D, K):
    """the scene of a shape, by a seed that is a function of the shape: the CPU test checks the one at (300, 333, 33, 3)"""
    return scene(9000 + 100000 * K + 1000 * D + 10 * ns + nt, ns, nt, D, K)


def tie_scene(ns, nt, D, K=3):
    """the shared scene with record 1 a copy of record 0: whatever record 1 admits, record 0 admits with the same residual"""
    sc = shared_scene(ns, nt, D, K)
    poses = sc.poses.copy()
    poses[1] = poses[0]
    return sc.with_poses(poses)


def shift(v):
    return AR.rt_of(np.eye(3), np.asarray(v, np.float64))


CLUSTER_A, CLUSTER_B, CLUSTER_FAR = np.array([0.0, 0, 0]), np.array([50.0, 0, 0]), np.array([0, 0, -90.0])


def cluster_scene(D=33, ns=130, nt=129):
    """(130, 129): two row blocks x three column tiles.  Every source row sits in cluster A.  Target columns 0..63 sit near A
    (admissible under record 0, the identity), 64..127 near B (admissible under record 2, the shift A -> B, and under no other),
    128.. in a cluster no record reaches: that tile is dropped by every record.  Record 1 shifts A to where no target is."""
    ct = np.concatenate([np.tile(CLUSTER_A, (64, 1)), np.tile(CLUSTER_B, (64, 1)), np.tile(CLUSTER_FAR, (nt - 128, 1))])
    base = MG.clusters(311, np.tile(CLUSTER_A, (ns, 1)), ct, D)
    return Scene(base.src_pts, base.fsrc, base.tgt_pts, base.ftgt, [shift([0, 0, 0]), shift([0, 80.0, 0]), shift(CLUSTER_B)])


def two_tiles_scene(D=2, ns=5, nt=70000):
    """(5, 70 000): 1094 column tiles in 547 slices of two (as test_two_tiles_per_slice_one_skipped of the single-pose tests).  The
    target tiles cycle through A, B and a cluster no record reaches, so a slice holds a computed tile beside a skipped one in either
    order; the records are those of cluster_scene."""
    tile = np.arange(nt) // 64
    ct = np.where((tile % 3 == 0)[:, None], CLUSTER_A[None], np.where((tile % 3 == 1)[:, None], CLUSTER_B[None], CLUSTER_FAR[None]))
    base = MG.clusters(312, np.tile(CLUSTER_A, (ns, 1)), ct, D)
    return Scene(base.src_pts, base.fsrc, base.tgt_pts, base.ftgt, [shift([0, 0, 0]), shift([0, 80.0, 0]), shift(CLUSTER_B)])
