"""The semantics of sc_polish_batch (include/saccot.h), restated per problem on the references that exist and nothing else:
tests/polish_ref.py::iterate on the input record's Rt, then O.score and O.mask, plus the status, pass-through and stop rules.  The
reference of tests/test_gpu_polish_batch.py; every comparison against it is bit for bit.  Also the scenes those tests share, so that
tests/test_polish_batch_abi.py can check on the CPU that they are what they are used for.  `O` is oracle/oracle.py."""
import numpy as np

import batch_ref
import polish_ref

SC_OK, SC_EINVAL, SC_ENOHYP = batch_ref.SC_OK, batch_ref.SC_EINVAL, batch_ref.SC_ENOHYP
STOP_FIXED, STOP_DECLINED, STOP_MAX_ITER = 0, 1, 2
_STOP = {"fixed": STOP_FIXED, "declined": STOP_DECLINED, "max_iter": STOP_MAX_ITER}
RESULT_DTYPE = np.dtype([("Rt", np.float32, 12), ("status", np.int32), ("score0", np.uint32), ("score", np.uint32), ("iters", np.uint16),
                         ("stop", np.uint16)])  # sc_polish_batch_result
FIELDS = ("status", "score0", "score", "iters", "stop")


def one(O, src, tgt, rec, tau, score_mode=0, max_iter=16):
    """-> (record, mask) of one problem: src, tgt (n, 3); rec: its input record (status and Rt are read)."""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    n = src.shape[0]
    out = np.zeros((), RESULT_DTYPE)
    out["Rt"], out["stop"] = batch_ref.IDENT, STOP_DECLINED
    if int(rec["status"]) != SC_OK:  # passed through
        out["status"] = rec["status"]
        return out, np.zeros(n, np.uint8)
    rt0 = np.ascontiguousarray(rec["Rt"], np.float32)
    if not (np.isfinite(src).all() and np.isfinite(tgt).all() and np.isfinite(rt0).all()):
        out["status"] = SC_EINVAL
        return out, np.zeros(n, np.uint8)
    rt, iters, stop = polish_ref.iterate(O, src, tgt, rt0, tau, max_iter)
    out["status"], out["Rt"], out["iters"], out["stop"] = SC_OK, rt, iters, _STOP[stop]
    out["score0"] = int(O.score(src, tgt, rt0[None, :], tau, score_mode=score_mode)[0])
    out["score"] = int(O.score(src, tgt, rt[None, :], tau, score_mode=score_mode)[0])
    return out, O.mask(src, tgt, rt, tau).copy()


def batch(O, problems, recs, tau, score_mode=0, max_iter=16):
    """problems: list of (src, tgt); recs: their input records -> (records (B,), list of masks)."""
    out = np.zeros(len(problems), RESULT_DTYPE)
    masks = []
    for b, (s, t) in enumerate(problems):
        out[b], m = one(O, s, t, recs[b], tau, score_mode, max_iter)
        masks.append(m)
    return out, masks


# ---- the scenes the tests of sc_polish_batch share ---------------------------------------------------------------------------
T = 200
TAUS = (0.05, 0.02)
MAX_ITERS = (1, 2, 16)


def kw_of(tau):
    return dict(batch_ref.KW, tau=tau, max_triangles=T)


def mixed(pkg):
    """batch_ref.mixed plus one problem of n = 129: n = 3, 4, 63, 64, 65, 128, 129, 257, 512, 512 — the chunk ends of the 64-index
    summation, one and two chunks, and the maximum."""
    problems = batch_ref.mixed(pkg)
    k = [len(s) for s, _ in problems].index(128) + 1
    return problems[:k] + [batch_ref.scene(pkg, 129, .3)] + problems[k:]


def sparse(pkg):
    """-> (kw, src, tgt): the first 128 correspondences of polish_ref.sparse_scene (the C0 scene, 40 hypotheses, tau = 0.001: a
    hypothesis catches its own three vertices at best): a winner with SC_OK that explains fewer than 3 correspondences, so its first
    refit is declined."""
    kw, src, tgt = polish_ref.sparse_scene(pkg)
    return {k: kw[k] for k in ("sigma", "t_cmp", "tau", "min_len", "max_triangles")}, np.ascontiguousarray(src[:128]), np.ascontiguousarray(tgt[:128])
