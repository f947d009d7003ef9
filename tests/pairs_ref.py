"""The semantics of sc_match_pairs / sc_register_pairs_features / sc_polish_pairs_slots_device (include/saccot.h): pair p's outputs
are the packed entries' for problem p of the list EXPANDED into packed problems in list order.  So the reference expands (table,
pair list) and calls the composed references that exist — match_batch_ref.match_one / features_one and polish_batch_ref.one — per
pair, and nothing else.  The reference of tests/test_gpu_pairs.py; every comparison against it is bit for bit.  Also the table and
the pair list those tests share, so that tests/test_pairs_abi.py can check on the CPU that they are what they are used for."""
import numpy as np

import batch_ref
import match_batch_ref as M
import polish_batch_ref as PB

SC_OK, SC_EINVAL, SC_ENOHYP = batch_ref.SC_OK, batch_ref.SC_EINVAL, batch_ref.SC_ENOHYP
DIM = 33  # the last chunk of a descriptor is short (16 + 16 + 1)
KW = M.KW
ROW_TILE, FINISH_STEP = M.ROW_TILE, 256  # source rows of a distance tile; rows of one step of the finish kernel (sc_match_batch.hip)


def slots(set_off, pairs, knn):
    """the Python restatement of sc_pairs_layout: slot[p] = knn x the source rows of the pairs before p; (P + 1,) uint32"""
    set_off = np.asarray(set_off, np.int64); pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    ns = set_off[pairs[:, 0] + 1] - set_off[pairs[:, 0]]
    return np.concatenate([[0], np.cumsum(ns * knn)]).astype(np.uint32)


# ---- the table and the list the tests share --------------------------------------------------------------------------------------
# sets 0 .. 7: random keypoints, sizes at the ends of the 64-row tile and of the finish kernel's 256-row step
RANDOM_SIZES = (1, 2, 3, 63, 64, 65, 129, 257)
R1, R2, R3, R63, R64, R65, R129, R257 = range(8)
N_SCENES = len(M.FEATURE_SCENES)


def scene_src(k):  # sets 8 .. 27: the two sides of match_batch_ref.feature_scenes()[k]
    return 8 + 2 * k


def scene_tgt(k):
    return 9 + 2 * k


TIE_A, TIE_B = 8 + 2 * N_SCENES, 9 + 2 * N_SCENES  # small integers, duplicated rows: the index alone decides
EMPTY = 10 + 2 * N_SCENES  # no rows, referenced by no pair
N_SETS = EMPTY + 1

_S = {n: k for k, (n, _, _) in enumerate(M.FEATURE_SCENES)}  # scene index by its keypoints
# 26 pairs in no order: every scene against its own target; scene 65's and scene 128's TARGET shared with a second source (mutual
# matching: the column minima of the two pairs must not meet); R65 the source of four pairs and the target of three; a self pair; a
# pair twice; two pairs whose target has one row; the tie pair; both sizes above 128 on either side
PAIRS = np.array([
    (R65, R129), (scene_src(_S[65]), scene_tgt(_S[65])), (R257, R129), (scene_src(_S[2]), scene_tgt(_S[2])), (R63, R65),
    (R64, scene_tgt(_S[65])), (scene_src(_S[128]), scene_tgt(_S[128])), (R65, R1), (scene_src(_S[16]), scene_tgt(_S[16])), (R64, R64),
    (scene_src(_S[100]), scene_tgt(_S[128])), (R129, R65), (scene_src(_S[3]), scene_tgt(_S[3])), (R65, R129), (TIE_A, TIE_B),
    (scene_src(_S[12]), scene_tgt(_S[12])), (R1, R257), (scene_src(_S[33]), scene_tgt(_S[33])), (R257, R65), (R2, R1),
    (scene_src(_S[64]), scene_tgt(_S[64])), (R65, R257), (scene_src(_S[63]), scene_tgt(_S[63])), (R2, R3), (scene_src(_S[100]), scene_tgt(_S[100])),
    (R3, R2)], np.uint32)
OWN_SCENE = {p: (int(a) - 8) // 2 for p, (a, b) in enumerate(PAIRS) if 8 <= a < TIE_A and b == a + 1 and a % 2 == 0}  # pair -> its scene

_TABLE = None


def table():
    """-> dict(sets: [(pts (n, 3), feat (n, DIM))], pts (total, 3), feat (total, DIM), set_off (N_SETS + 1,) uint32, R: the scenes'
    rotations); built once, never modified"""
    global _TABLE
    if _TABLE is None:
        sets = []
        for n in RANDOM_SIZES:
            rng = np.random.default_rng(9000 + n)
            sets.append((rng.uniform(-1, 1, size=(n, 3)).astype(np.float32), rng.normal(size=(n, DIM)).astype(np.float32)))
        scenes = M.feature_scenes()
        for s in scenes:
            assert s[1].shape[1] == DIM
            sets += [(s[0], s[1]), (s[2], s[3])]
        rng = np.random.default_rng(55)
        base = np.zeros((4, DIM), np.float32)
        base[:, [0, 16, 32]] = rng.integers(-2, 3, size=(4, 3)).astype(np.float32)  # a component in every chunk
        for n in (70, 66):
            sets.append((rng.uniform(-1, 1, size=(n, 3)).astype(np.float32), base[rng.integers(0, 4, n)]))
        sets.append((np.zeros((0, 3), np.float32), np.zeros((0, DIM), np.float32)))
        assert len(sets) == N_SETS
        set_off = np.concatenate([[0], np.cumsum([len(p) for p, _ in sets])]).astype(np.uint32)
        _TABLE = dict(sets=sets, pts=np.concatenate([p for p, _ in sets]), feat=np.concatenate([f for _, f in sets]), set_off=set_off,
                      R=[s[4] for s in scenes])
    return _TABLE


def expand(tab, pairs):
    """the pair list as packed problems in list order: [(src_pts, fsrc, tgt_pts, ftgt)] — what a caller of sc_match_batch builds"""
    return [(tab["sets"][a][0], tab["sets"][a][1], tab["sets"][b][0], tab["sets"][b][1]) for a, b in np.asarray(pairs).reshape(-1, 2)]


def with_sets(tab, changed):
    """a copy of the table with some sets replaced: changed = {set index: (pts, feat)} of the same sizes"""
    sets = [changed.get(s, v) for s, v in enumerate(tab["sets"])]
    return dict(tab, sets=sets, pts=np.concatenate([p for p, _ in sets]), feat=np.concatenate([f for _, f in sets]))


# ---- the reference: per pair, on its two sets alone ------------------------------------------------------------------------------------
def match(tab, pairs, mkw):
    """-> [(corr, d2, n, flag)] per pair"""
    memo = {}
    out = []
    for a, b in np.asarray(pairs).reshape(-1, 2).tolist():
        if (a, b) not in memo:
            memo[a, b] = M.match_one(tab["sets"][a][1], tab["sets"][b][1], **mkw)
        out.append(memo[a, b])
    return out


def features(O, tab, pairs, mkw, kw, score_mode=0):
    """-> [dict(corr, d2, n, flag, rec, mask)] per pair"""
    memo = {}
    out = []
    for a, b in np.asarray(pairs).reshape(-1, 2).tolist():
        if (a, b) not in memo:
            (ps, fs), (pt, ft) = tab["sets"][a], tab["sets"][b]
            memo[a, b] = M.features_one(O, ps, fs, pt, ft, mkw, kw, score_mode)
        out.append(memo[a, b])
    return out


def polish(O, tab, pairs, feats, tau, score_mode=0, max_iter=16):
    """feats: features() of the same list -> [(record, mask)] per pair: polish_batch_ref.one on the gathered correspondences with
    the pair's record as input (a flagged or short pair passes its status through)"""
    out = []
    for (a, b), f in zip(np.asarray(pairs).reshape(-1, 2).tolist(), feats):
        gs = tab["sets"][a][0][f["corr"][:, 0]]
        gt = tab["sets"][b][0][f["corr"][:, 1]]
        out.append(PB.one(O, gs, gt, f["rec"], tau, score_mode, max_iter))
    return out
