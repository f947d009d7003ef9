"""The semantics of sc_register_batch (include/saccot.h), restated on the CPU restatement's whole path and nothing else: problem b's
record and mask are what O.register returns for problem b alone.  The reference of tests/test_gpu_batch.py.  `O` is oracle/oracle.py."""
import numpy as np

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
_STATUS = {0: SC_OK, -1: SC_EINVAL, -5: SC_ENOHYP}  # the restatement's SO_* codes -> the library's
RESULT_DTYPE = np.dtype([("Rt", np.float32, 12), ("status", np.int32), ("n", np.uint32), ("edges", np.uint32), ("tri_kept", np.uint32),
                         ("tri_total", np.uint64), ("best_rank", np.uint32), ("best_count", np.uint32)])  # sc_batch_result
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
TRI_CAP = 200_000  # the tests' condition: no problem of theirs holds more triangles (a workgroup's run time)


def one(O, src, tgt, kw, score_mode=0):
    """-> (record, mask) of one problem: src, tgt (n, 3).  kw: sigma, t_cmp, tau, min_len, max_triangles, rank_mode."""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    n = src.shape[0]
    rec = np.zeros((), RESULT_DTYPE)
    rec["Rt"], rec["n"] = IDENT, n
    if not (np.isfinite(src).all() and np.isfinite(tgt).all()):  # the finiteness rule: found per problem, every count 0
        rec["status"] = SC_EINVAL
        return rec, np.zeros(n, np.uint8)
    r = O.register(src, tgt, kw["sigma"], kw["t_cmp"], kw["tau"], kw["min_len"], kw["max_triangles"], kw.get("rank_mode", 0),
                   threads=1, score_mode=score_mode)
    rec["status"] = _STATUS[r["rc"]]
    rec["Rt"] = np.concatenate([r["R"].ravel(), r["t"]])
    for f, k in (("edges", "edges"), ("tri_total", "tri_total"), ("tri_kept", "t_eff"), ("best_rank", "best_rank"), ("best_count", "best_count")):
        rec[f] = r[k]
    return rec, r["mask"].copy()


def batch(O, problems, kw, score_mode=0):
    """problems: list of (src, tgt) -> (records (B,), list of masks)."""
    recs = np.zeros(len(problems), RESULT_DTYPE)
    masks = []
    for b, (s, t) in enumerate(problems):
        recs[b], m = one(O, s, t, kw, score_mode)
        masks.append(m)
    return recs, masks


# ---- the scenes the tests of sc_register_batch share -------------------------------------------------------------------------
KW = dict(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05)
MIXED = ((3, 1.0), (4, 1.0), (63, .3), (64, .3), (65, .3), (128, .3), (257, .25), (512, .2), (512, .3))


def scene(pkg, n, rho, seed=None):
    sc = pkg.synth.make_scene(n, rho, 1.0, 0.05, 7000 + n if seed is None else seed)
    return sc.src, sc.tgt


def mixed(pkg):
    return [scene(pkg, n, rho) for n, rho in MIXED]


def exact_scene():
    """40 points on the grid integers(-512, 512) / 64, tgt = src + (2, -1, 0.5): every length is exact in fp32 and equal on both
    sides, so every weight is exactly 1 and every key equal — (i, j, k) alone decides the cut and the winner's rank."""
    rng = np.random.default_rng(40)
    src = (rng.integers(-512, 512, size=(40, 3)) / 64).astype(np.float32)
    return src, (src + np.array([2, -1, 0.5], np.float32)).astype(np.float32)
