"""The semantics of sc_polish (include/saccot.h), restated in numpy on the CPU restatement's stage functions and nothing else
(O.score, O.mask, O.refine): the reference of tests/test_gpu_polish.py.  `O` is oracle/oracle.py."""
import numpy as np

SC_OK, SC_ENOHYP = 0, -5
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def hypotheses(O, src, tgt, kw, threads=1):
    """Stage A -> ranked list -> Kabsch: the frame's T hypotheses in ranked order, and the frame's counts."""
    S, bits, deg = O.compat(src, tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"], threads=threads)
    tri, key, total = O.triangles(S, bits, deg, kw["max_triangles"], kw.get("rank_mode", 0), threads=threads)
    return dict(Rt=O.kabsch3(src, tgt, tri, threads=threads), t_eff=len(tri), total=total, edges=int(deg.sum()) // 2)


def candidates(cnt, k):
    """Positions of the first min(k, #score > 0) hypotheses under (score descending, position in the ranked list ascending)."""
    cnt = np.asarray(cnt, np.uint32)
    key = (cnt.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(len(cnt), dtype=np.uint64))
    order = np.argsort(key, kind="stable")[::-1]
    return [int(g) for g in order[: min(k, int((cnt > 0).sum()))]]


def iterate(O, src, tgt, rt0, tau, max_iter):
    """-> (last iterate, refits that changed (R, t), how it stopped: "declined" | "fixed" | "max_iter")."""
    rt = np.ascontiguousarray(rt0, np.float32).reshape(12).copy()
    iters = 0
    for _ in range(max_iter):
        mask = O.mask(src, tgt, rt, tau)
        done, rt2 = O.refine(src, tgt, mask, rt)
        if not done:
            return rt, iters, "declined"
        if rt2.tobytes() == rt.tobytes():
            return rt, iters, "fixed"
        rt = rt2
        iters += 1
    return rt, iters, "max_iter"


def polish(O, src, tgt, Rt, tau, score_mode=0, candidates_=8, max_iter=16, cnt=None, threads=1):
    """Rt: the frame's hypotheses in ranked order (T x 12).  cnt: their frame scores (computed when None).
    -> dict(status, cand: list of dict(Rt, rank, score0, score, iters, stop), winner: index into cand, Rt, mask, best_rank, best_count)."""
    n = src.shape[0]
    if cnt is None:
        cnt = O.score(src, tgt, Rt, tau, threads=threads, score_mode=score_mode)
    cand = []
    for g in candidates(cnt, candidates_):
        rt, iters, stop = iterate(O, src, tgt, Rt[g], tau, max_iter)
        score = int(O.score(src, tgt, rt[None, :], tau, score_mode=score_mode)[0])
        cand.append(dict(Rt=rt, rank=g, score0=int(cnt[g]), score=score, iters=iters, stop=stop))
    if not cand:
        return dict(status=SC_ENOHYP, cand=[], winner=None, Rt=IDENT.copy(), mask=np.zeros(n, np.uint8), best_rank=0, best_count=0)
    w = max(range(len(cand)), key=lambda i: (cand[i]["score"], -i))  # largest score, ties to the earlier candidate
    return dict(status=SC_OK, cand=cand, winner=w, Rt=cand[w]["Rt"], mask=O.mask(src, tgt, cand[w]["Rt"], tau),
                best_rank=cand[w]["rank"], best_count=cand[w]["score"])


# ---- the scenes the tests of sc_polish share beside the configs' own ------------------------------------------------------
def edge_scene(pkg, n):
    """The first n correspondences of the C0 scene reordered so that its true correspondences come first (both groups in index
    order): n = 64, 65, 129 put the end of the input on, one past and one past the second of the refit's 64-index chunks."""
    cfg, sc = pkg.synth.make_config_scene("C0")
    idx = np.concatenate([np.flatnonzero(sc.inlier), np.flatnonzero(~sc.inlier)])[:n]
    return cfg.params(), np.ascontiguousarray(sc.src[idx]), np.ascontiguousarray(sc.tgt[idx])


def sparse_scene(pkg):
    """The C0 scene with 40 hypotheses and tau = 0.001, a fiftieth of the rigidity scale the triangles were chosen by: a
    hypothesis catches its own three vertices at best, so most scores are 1 .. 3 and some are 0 — fewer candidates than a caller
    asks for, and candidates whose refit is declined (fewer than 3 inliers)."""
    cfg, sc = pkg.synth.make_config_scene("C0")
    kw = cfg.params()
    kw.update(tau=0.001, max_triangles=40)
    return kw, sc.src, sc.tgt
