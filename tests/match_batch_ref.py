"""The semantics of sc_match_batch / sc_register_batch_features (include/saccot.h), composed per problem from the two references
that exist: tests/match_ref.py (the canonical matcher in numpy float32), a gather, and tests/batch_ref.py (one problem through the
CPU restatement).  The reference of tests/test_gpu_match_batch.py; every comparison against it is bit for bit.  Also the scenes
those tests share, so that tests/test_match_batch_abi.py can check on the CPU that they are what they are used for."""
import numpy as np

import batch_ref
import match_ref

SC_OK, SC_EINVAL, SC_ENOHYP = batch_ref.SC_OK, batch_ref.SC_EINVAL, batch_ref.SC_ENOHYP
ROW_TILE = 64  # source rows of a workgroup's tile (sc_match_batch.hip): the mixed batch has sizes one row either side of it


def match_one(fsrc, ftgt, knn=1, mutual=False, ratio=0.0):
    """-> (corr (n, 2) int32, d2 (n,) float32, n, flag) of sc_match on one problem; a non-finite descriptor: flag 1, n 0."""
    fsrc, ftgt = np.asarray(fsrc, np.float32), np.asarray(ftgt, np.float32)
    if not (np.isfinite(fsrc).all() and np.isfinite(ftgt).all()):
        return np.zeros((0, 2), np.int32), np.zeros(0, np.float32), 0, 1
    corr, d2 = match_ref.match(fsrc, ftgt, knn=knn, mutual=mutual, ratio=ratio)
    return corr, d2, len(corr), 0


def features_one(O, src_pts, fsrc, tgt_pts, ftgt, mkw, kw, score_mode=0):
    """-> dict(corr, d2, n, flag, rec, mask) of one problem of sc_register_batch_features: match, gather, batch_ref.one."""
    corr, d2, n, flag = match_one(fsrc, ftgt, **mkw)
    rec = np.zeros((), batch_ref.RESULT_DTYPE)
    rec["Rt"] = batch_ref.IDENT
    if flag:
        rec["status"], rec["n"] = SC_EINVAL, 0
        mask = np.zeros(0, np.uint8)
    elif n < 3:
        rec["status"], rec["n"] = SC_ENOHYP, n
        mask = np.zeros(n, np.uint8)
    else:
        gs = np.asarray(src_pts, np.float32)[corr[:, 0]]
        gt = np.asarray(tgt_pts, np.float32)[corr[:, 1]]
        rec, mask = batch_ref.one(O, gs, gt, kw, score_mode)
    return dict(corr=corr, d2=d2, n=n, flag=flag, rec=rec, mask=mask)


# ---- the scenes the tests share ----------------------------------------------------------------------------------------------
MIXED_SIZES = ((1, 1), (1, 5), (5, 1), (3, 2), (63, 65), (64, 64), (65, 63), (127, 129), (128, 128), (129, 257), (300, 200))
MIXED_DIMS = (1, 15, 16, 17, 33)
MATCH_MODES = (dict(knn=1), dict(knn=2), dict(knn=3), dict(knn=4), dict(knn=1, mutual=True), dict(knn=1, ratio=0.8),
               dict(knn=1, mutual=True, ratio=0.8))


def mixed_descriptors(dim, sizes=MIXED_SIZES):
    """one (fsrc, ftgt) per size: normal descriptors; the first min(ns, nt) target rows are noisy copies of source rows"""
    out = []
    for k, (ns, nt) in enumerate(sizes):
        rng = np.random.default_rng(1000 * dim + k)
        a = rng.normal(size=(ns, dim)).astype(np.float32)
        b = rng.normal(size=(nt, dim)).astype(np.float32)
        m = min(ns, nt)
        b[:m] = a[rng.permutation(ns)[:m]] + np.float32(0.1) * rng.normal(size=(m, dim)).astype(np.float32)
        out.append((a, b))
    return out


def tie_descriptors():
    """small integers, rows duplicated on both sides: equal distances in a row and in a column — the index alone decides"""
    rng = np.random.default_rng(5)
    out = []
    for ns, nt in ((9, 7), (70, 66), (5, 130)):
        base = rng.integers(-2, 3, size=(4, 3)).astype(np.float32)
        out.append((base[rng.integers(0, 4, ns)], base[rng.integers(0, 4, nt)]))
    return out


KW = dict(batch_ref.KW, max_triangles=200)
# (keypoints, inlier ratio, noise): two keypoints (n_b < 3), three exact ones (n_b == 3), outliers only (no consistent triangle),
# then sizes up to 128 — one either side of a wave, of the row tile, and the largest
FEATURE_SCENES = ((2, 1.0, 0.0), (3, 1.0, 0.0), (12, 0.0, 0.0), (16, 0.8, 0.001), (33, 0.6, 0.001), (63, 0.5, 0.001), (64, 0.5, 0.001),
                  (65, 0.5, 0.001), (100, 0.4, 0.001), (128, 0.4, 0.001))


def feature_scene(n, rho, noise, seed, dim=33):
    """-> (src_pts, fsrc, tgt_pts, ftgt, R): n keypoints a side.  An inlier's target point is R p + t (+ noise) and its target
    descriptor the source descriptor plus small noise; an outlier's are random.  The target order is shuffled."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1, 1, size=(n, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    R = q * np.sign(np.linalg.det(q))
    t = rng.uniform(-1, 1, size=3)
    n_in = int(round(rho * n))
    tgt = src @ R.T + t + noise * rng.normal(size=(n, 3))
    tgt[n_in:] = rng.uniform(-2, 2, size=(n - n_in, 3))
    fsrc = rng.normal(size=(n, dim))
    ftgt = fsrc + 0.05 * rng.normal(size=(n, dim))
    ftgt[n_in:] = rng.normal(size=(n - n_in, dim))
    perm = rng.permutation(n)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return f32(src), f32(fsrc), f32(tgt[perm]), f32(ftgt[perm]), R


def feature_scenes():
    return [feature_scene(n, rho, noise, 4000 + n) for n, rho, noise in FEATURE_SCENES]


def rotation_error_deg(R, R_true):
    c = (np.trace(np.asarray(R, np.float64).reshape(3, 3) @ R_true.T) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))
