"""The semantics of sc_match_guided (include/saccot.h), restated in numpy: the reference of tests/test_gpu_match_guided.py; every
comparison against it is bit for bit.  The descriptor distance is match_ref.distances; the gate residual and its threshold are
assign_ref.resid2 / tau2_of (the exact fp32 fma emulation), evaluated on ALL ns x nt pairs; the selection is match_ref's with every
inadmissible key replaced by all ones.  Also the scenes the tests share, so that the CPU test can check what they are used for."""
import numpy as np

import assign_ref as AR
import match_ref

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
MODES = [dict(knn=1), dict(knn=2), dict(knn=3), dict(knn=4), dict(knn=1, mutual=True), dict(knn=1, ratio=0.8), dict(knn=1, ratio=0.9999)]
GATE = 0.15          # the gate of the shared scenes (source points fill the unit cube)
GATE_NOTHING = 1e-6  # ... and one that admits no pair of them (the planted pairs are about 1e-2 apart)
GATE_ALL = 1e18      # ... and one that admits every pair of points of moderate size (gate2 = 1e36 is finite)


def gate2_of(gate):
    with np.errstate(over="ignore"):
        return AR.tau2_of(gate)


def gate_residuals(Rt, src_pts, tgt_pts):
    """g2(i, j) = resid2(Rt, src_pts[i], tgt_pts[j]) for every pair: (ns, nt) float32"""
    src_pts, tgt_pts = np.ascontiguousarray(src_pts, np.float32).reshape(-1, 3), np.ascontiguousarray(tgt_pts, np.float32).reshape(-1, 3)
    ns, nt = len(src_pts), len(tgt_pts)
    out = np.empty((ns, nt), np.float32)
    step = max(1, 400000 // nt)
    for lo in range(0, ns, step):
        hi = min(ns, lo + step)
        out[lo:hi] = AR.resid2(Rt, np.repeat(src_pts[lo:hi], nt, axis=0), np.tile(tgt_pts, (hi - lo, 1))).reshape(hi - lo, nt)
    return out


def admissible(g2, gate):
    with np.errstate(invalid="ignore"):
        return g2 < gate2_of(gate)  # a float <: NaN and inf are never admissible


def select(acc, g2, adm, knn=1, mutual=False, ratio=0.0):
    """the masked selection -> (corr (n, 2) int32, d2 (n,), g2 (n,)) in ascending (source row, rank) order"""
    ns, nt = acc.shape
    hi = acc.view(np.uint32).astype(np.uint64) << np.uint64(32)
    key = np.where(adm, hi | np.arange(nt, dtype=np.uint64)[None, :], KEY_NONE)
    rkey = np.where(adm, hi | np.arange(ns, dtype=np.uint64)[:, None], KEY_NONE)
    order = np.argsort(key, axis=1, kind="stable")
    skey = np.take_along_axis(key, order, axis=1)
    keep = skey[:, :min(knn, nt)] != KEY_NONE  # fewer where fewer are admissible
    if mutual or ratio > 0:
        assert knn == 1
        rows, j = np.arange(ns), order[:, 0]
        if mutual:
            keep[:, 0] &= np.argmin(rkey, axis=0)[j] == rows  # target j's minimum over its admissible i only
        if ratio > 0 and nt > 1:
            r = np.float32(ratio)
            r2 = np.float32(np.float64(r) * np.float64(r))
            with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                passed = acc[rows, j] < r2 * acc[rows, order[:, 1]]
            keep[:, 0] &= passed | (skey[:, 1] == KEY_NONE)  # kept with fewer than two admissible candidates
    i_idx, rank = np.nonzero(keep)
    j_idx = order[i_idx, rank]
    corr = np.stack([i_idx, j_idx], axis=1).astype(np.int32).reshape(-1, 2)
    return corr, acc[i_idx, j_idx].astype(np.float32), g2[i_idx, j_idx].astype(np.float32)


class Problem:
    """one (scene, pose, gate): the distances, the residuals and the mask are computed once and shared by the modes"""

    def __init__(self, src_pts, fsrc, tgt_pts, ftgt, Rt, gate):
        self.acc = match_ref.distances(fsrc, ftgt)
        self.g2 = gate_residuals(Rt, src_pts, tgt_pts)
        self.adm = admissible(self.g2, gate)

    def match(self, **kw):
        return select(self.acc, self.g2, self.adm, **kw)


def match(src_pts, fsrc, tgt_pts, ftgt, Rt, gate, **kw):
    return Problem(src_pts, fsrc, tgt_pts, ftgt, Rt, gate).match(**kw)


# ---- the scenes the tests share ----------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, src_pts, fsrc, tgt_pts, ftgt, Rt):
        self.src_pts, self.fsrc, self.tgt_pts, self.ftgt, self.Rt = src_pts, fsrc, tgt_pts, ftgt, Rt

    def args(self):
        return self.src_pts, self.fsrc, self.tgt_pts, self.ftgt, self.Rt


def random_pose(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q, rng.standard_normal(3) * 0.5


def scene(seed, ns, nt, D, sd=0.3, noise=0.01):
    """source points in the unit cube; a random rotation and translation; the first third of the target rows are posed copies of
    source rows with small point noise and noisy descriptor copies (as _descriptors of test_gpu_match.py plants them); the remaining
    target rows are random in the posed cube with random descriptors"""
    rng = np.random.default_rng(seed)
    src = rng.random((ns, 3))
    R, t = random_pose(rng)
    tgt = rng.random((nt, 3)) @ R.T + t
    fsrc = rng.standard_normal((ns, D)).astype(np.float32)
    ftgt = rng.standard_normal((nt, D)).astype(np.float32)
    m = min(ns, nt // 3)
    if m:
        rows = rng.permutation(ns)[:m]
        tgt[:m] = src[rows] @ R.T + t + noise * rng.standard_normal((m, 3))
        ftgt[:m] = fsrc[rows] + np.float32(sd) * rng.standard_normal((m, D)).astype(np.float32)
    return Scene(src.astype(np.float32), fsrc, tgt.astype(np.float32), ftgt, AR.rt_of(R, t))


def shared_scene(ns, nt, D):
    """the scene of a shape, by a seed that is a function of the shape: the CPU test checks the one at (300, 333, 33)"""
    return scene(7000 + 1000 * D + 10 * ns + nt, ns, nt, D)


def clusters(seed, centres_src, centres_tgt, D, spread=0.05):
    """Keypoints in far clusters under the identity pose: centres_src / centres_tgt give every row's cluster centre ((n, 3) arrays;
    centres are tens of gates apart), rows scatter `spread` around them; random descriptors.  Which tiles drop out follows from
    which row ranges share a centre."""
    rng = np.random.default_rng(seed)
    cs, ct = np.asarray(centres_src, np.float64), np.asarray(centres_tgt, np.float64)
    src = cs + spread * rng.standard_normal(cs.shape)
    tgt = ct + spread * rng.standard_normal(ct.shape)
    fsrc = rng.standard_normal((len(cs), D)).astype(np.float32)
    ftgt = rng.standard_normal((len(ct), D)).astype(np.float32)
    ident = AR.rt_of(np.eye(3), np.zeros(3))
    return Scene(src.astype(np.float32), fsrc, tgt.astype(np.float32), ftgt, ident)
