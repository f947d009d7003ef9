"""The semantics of sc_register_instances_batch (include/saccot.h), composed per problem from the CPU restatement and nothing else:
plane 0 is tests/batch_ref.py's record of the problem (the whole path), and the motions are stage A -> the ranked list -> the Kabsch
stage once, then per round the scores of every kept hypothesis over the unclaimed correspondences, the winner by the frame's total
order, its mask among the unclaimed — the composition tests/test_gpu_peel.py::_expected uses — plus min_score, the label, nfound and
the shaped empty planes.  The reference of tests/test_gpu_instances_batch.py; every comparison against it is bit for bit.  Also the
scenes those tests share, so that tests/test_instances_batch_abi.py can check on the CPU that they are what they are used for."""
import numpy as np

import batch_ref

SC_OK, SC_EINVAL, SC_ENOHYP = batch_ref.SC_OK, batch_ref.SC_EINVAL, batch_ref.SC_ENOHYP
KW = batch_ref.KW
# (n, rho): one bit word and its neighbours, one and two 256-thread strides, the maximum; 3 and 4 hold no triangle
SCENES = ((3, 1.0), (4, 1.0), (63, .5), (64, .5), (65, .5), (128, .5), (257, .4), (512, .3))


def scene(pkg, n, rho):
    """two motions: 0.6 rho and 0.4 rho of the n correspondences"""
    sc = pkg.synth.make_scene_motions(n, [0.6 * rho, 0.4 * rho], 1.0, 0.05, 7100 + n)
    return sc.src, sc.tgt


def scenes(pkg):
    return [scene(pkg, n, rho) for n, rho in SCENES]


def empty_plane(rec0):
    """a plane without a motion: plane 0's counts, R = I, t = 0, SC_ENOHYP unless the problem itself is SC_EINVAL"""
    e = rec0.copy()
    e["Rt"], e["best_rank"], e["best_count"] = batch_ref.IDENT, 0, 0
    e["status"] = SC_EINVAL if rec0["status"] == SC_EINVAL else SC_ENOHYP
    return e


def rounds(O, src, tgt, kw, score_mode, rec0, max_instances, min_score, info=None):
    """-> (planes (max_instances,), label (n,) int32, nfound) given plane 0's record rec0.  info: a dict that receives `winners`, the
    (i, j, k) of every found motion's triangle, `claimed_vertex`, whether a round's winner had a claimed vertex, and `end`, why the rounds
    ended: ("min_score", the best score left, below it) or ("max_instances", max_instances)."""
    n = len(src)
    planes = np.zeros(max_instances, batch_ref.RESULT_DTYPE)
    planes[0] = rec0
    planes[1:] = empty_plane(rec0)
    label = np.full(n, -1, np.int32)
    if rec0["status"] != SC_OK or rec0["best_count"] < min_score:
        return planes, label, 0
    S, bits, deg = O.compat(src, tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"], threads=1)
    tri, key, total = O.triangles(S, bits, deg, kw["max_triangles"], kw.get("rank_mode", 0), threads=1)
    Rt = O.kabsch3(src, tgt, tri, threads=1)
    alive = np.ones(n, bool)
    found = 0
    for k in range(max_instances):
        cnt = (O.score(src[alive], tgt[alive], Rt, kw["tau"], threads=1, score_mode=score_mode) if alive.any()
               else np.zeros(len(Rt), np.uint32))
        best_key = O.best_key(cnt)
        if best_key == 0 or (best_key >> 32) < min_score:
            if info is not None:
                info["end"] = ("min_score", int(best_key >> 32))
            break
        best = 0xFFFFFFFF - (best_key & 0xFFFFFFFF)
        m = O.mask(src, tgt, Rt[best], kw["tau"]).astype(bool) & alive
        if info is not None:
            info.setdefault("winners", []).append(tuple(int(x) for x in tri[best]))
            if k and not alive[np.asarray(tri[best], np.int64)].all():
                info["claimed_vertex"] = True
        if k == 0:  # the frame itself: what batch_ref.one returned for the whole path
            assert best == rec0["best_rank"] and (best_key >> 32) == rec0["best_count"] and Rt[best].tobytes() == rec0["Rt"].tobytes()
        else:
            planes[k] = rec0
            planes[k]["Rt"], planes[k]["best_rank"], planes[k]["best_count"] = Rt[best], best, best_key >> 32
        label[m] = k
        alive &= ~m
        found = k + 1
    else:
        if info is not None:
            info["end"] = ("max_instances", max_instances)
    return planes, label, found


def one(O, src, tgt, kw, score_mode=0, max_instances=4, min_score=4, info=None):
    """-> (planes, label, nfound) of one problem: src, tgt (n, 3)"""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    rec0, _ = batch_ref.one(O, src, tgt, kw, score_mode)
    return rounds(O, src, tgt, kw, score_mode, rec0, max_instances, min_score, info)


def batch(O, problems, kw, score_mode=0, max_instances=4, min_score=4):
    """problems: list of (src, tgt) -> (records (max_instances, B) motion-major, list of labels, nfound (B,))"""
    recs = np.zeros((max_instances, len(problems)), batch_ref.RESULT_DTYPE)
    labels, nfound = [], np.zeros(len(problems), np.uint32)
    for b, (s, t) in enumerate(problems):
        recs[:, b], lab, nfound[b] = one(O, s, t, kw, score_mode, max_instances, min_score)
        labels.append(lab)
    return recs, labels, nfound
