"""CPU suite: the inputs of tests/test_gpu_settle_range.py and tests/test_gpu_merge_range.py — sc_settle_poses and sc_merge_poses
(frame and batch forms) at the ends of the fp32 range and past one trip of their loops — and what the REFERENCES alone say about
them.

The two GPU files compare the kernels with tests/settle_ref.py and tests/merge_ref.py bit for bit: the 64 bytes of every record,
every label, the bits of every d2, every parent, every overlap cell, the count words and the rounds words.  That is only worth
something if the inputs leave the beaten path for the reason meant, and all of that is asserted here, on the references alone.  This
file owns the case tables and the cached reference results (once per session, never modified); frames, batch problems and pose lists
are those of tests/test_pose_range_ref.py, test_batch_range_ref.py, test_batch_tail_range_ref.py and test_range_oracle.py (imported,
not copied).

Frames: test_pose_range_ref.FRAME_CASES through frame_case — scene_small (n = 300) times 2^k, far from the origin, rows at +-3e38,
tau at the ends of its range, the truncated score modes, the sparse scene (n = 500), scene_big (n = 1500) at k = 62 and -56 — and
the one NO_FRAME case.  Pose lists per frame:
  K3    assign_poses(...)["K3"]: two neighbours of the winner and a copy of the first, bare floats at stride 48;
  K12   frame_poses: the ten POLISH_POSES and the winner under status -1 and -5, records of 64 bytes under the status flag;
  K65   the hostile and status positions of pose_lists; its first 64 go to settle as K64 (SC_SETTLE_MAX_POSES), the whole to merge;
  near  the big frames only: the winner shifted by fractions of tau and turned about its inliers' centroid (on K12 and K64 those
        frames settle in one round: neighbours that turn about the origin fit nothing 2^62 away from it).

Shapes at unit scale: merge_ref.scene at n = 2048, 2049, 2113 — merge_overlap_kernel streams 32 words (2048 correspondences) of a
bit row at a time, a trip of settle_label covers 32 chunks: one word past, and a partial second pass — with merge_ref.many's lists,
K = 33 for merge and K = 8 for settle.  Decide rounds on the n = 129 frame: K = 65, 127, 128, 129, 130; in the K = 130 list 72
entries are exact copies of the list's strongest pose, numbered below and above it, so that the tied ranks straddle rank 63 | 64
and "ties go to the lower pose number" is what decides the parent; and a call whose min_count exceeds every count.

Batches: test_pose_range_ref.ASSIGN_LAUNCHES (at most 40 problems a launch, n <= 512) with assign_batch_poses; settle takes K = 1,
3, 16 (SC_SETTLE_BATCH_MAX_POSES), merge K = 1, 3, 16, 64.
"""
import numpy as np

import assign_ref as AR
import merge_ref as MR
import settle_ref as SR
import test_batch_range_ref as R
import test_batch_tail_range_ref as TR
import test_pose_range_ref as P
from test_range_oracle import pow2

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
FIXED, DECLINED, MAX_ITER = SR.STOP_FIXED, SR.STOP_DECLINED, SR.STOP_MAX_ITER
SETTLE_MAX_POSES, SETTLE_BATCH_MAX_POSES = 64, 16      # SC_SETTLE_MAX_POSES, SC_SETTLE_BATCH_MAX_POSES
_REF = {}

FRAME_CASES, NO_FRAME, IN_WINDOW_FRAMES = P.FRAME_CASES, P.NO_FRAME, P.IN_WINDOW_FRAMES
BIG_FRAMES = [name for name in FRAME_CASES if name.startswith("big:")]
COUNT_FRAMES = [name for name in IN_WINDOW_FRAMES if name.startswith("a:") and name.count(":") == 1]   # family a, score mode 0
MODE_FRAMES = [name for name in IN_WINDOW_FRAMES if name.count(":") == 2]                              # a:k:mode1 / mode2


# ================================================================================================================================
# frames: the pose lists and the runs
# ================================================================================================================================
NEAR_SHIFTS = ("shift:0.3", "shift:-0.3", "shift:0.6")    # test_batch_tail_range_ref.pose_of on the winner
NEAR_TURNS, NEAR_SEED = 8, 1501                           # ... and seeded turns about the inliers' centroid
NEAR_ANGLE = 0.05                                         # radians: 0.05 x the scene's radius (about 0.5) is half of tau


def near_list(pkg, O, name):
    """the list `near` of a big frame: K = 11 neighbours of the winner that share its inliers and trade them for rounds"""
    src, tgt, kw, mode, frame = P.frame_case(pkg, O, name)
    w = P.winner_of(frame)
    out = [TR.pose_of(w, kw["tau"], s) for s in NEAR_SHIFTS]
    Rw, tw = w[:9].astype(np.float64).reshape(3, 3), w[9:].astype(np.float64)
    c = tgt[np.asarray(frame["mask"]) != 0].astype(np.float64).mean(axis=0)
    rng = np.random.default_rng(NEAR_SEED)
    for _ in range(NEAR_TURNS):
        v = rng.normal(size=3)
        v *= NEAR_ANGLE / np.linalg.norm(v)
        th = np.linalg.norm(v)
        Kx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        dR = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)
        out.append(AR.rt_of(dR @ Rw, dR @ (tw - c) + c))  # q -> dR (q - c) + c behind the winner
    return np.ascontiguousarray(np.stack(out), np.float32)


def frame_lists(pkg, O, name):
    """-> {list name: (Rt (K, 12), statuses (K,) or None)}; a list without statuses goes in as bare floats at stride 48"""
    key = ("lists", name)
    if key not in _REF:
        ap = P.assign_poses(pkg, O, name)
        rt65, st65 = ap["K65"]
        out = {"K3": ap["K3"], "K12": P.frame_poses(pkg, O, name), "K65": (rt65, st65),
               "K64": (np.ascontiguousarray(rt65[:SETTLE_MAX_POSES]), st65[:SETTLE_MAX_POSES].copy())}
        if name in BIG_FRAMES:
            out["near"] = (near_list(pkg, O, name), None)
        _REF[key] = out
    return _REF[key]


# settle: (list, max_iter, masked)
SETTLE_RUNS = [("K12", 1, False), ("K12", 2, False), ("K12", 16, False), ("K12", 16, True), ("K3", 16, False), ("K3", 16, True),
               ("K64", 16, False), ("K64", 16, True)]
SETTLE_PARTS = ("K12", "K3", "K64")
NEAR_RUNS = [("near", 2, False), ("near", 16, False), ("near", 16, True)]


def settle_runs(name, part):
    return [r for r in SETTLE_RUNS + (NEAR_RUNS if name in BIG_FRAMES else []) if r[0] == part]


def settle_parts(name):
    return SETTLE_PARTS + (("near",) if name in BIG_FRAMES else ())


def settle_ref(pkg, O, name, which, max_iter, masked=False):
    """-> (records, label, d2, rounds) of settle_ref.settle on the frame under the frame's own score mode"""
    key = ("settle", name, which, max_iter, masked)
    if key not in _REF:
        src, tgt, kw, mode, frame = P.frame_case(pkg, O, name)
        rt, st = frame_lists(pkg, O, name)[which]
        with np.errstate(all="ignore"):
            _REF[key] = SR.settle(O, src, tgt, rt, kw["tau"], P.third_off(len(src)) if masked else None, st, mode, max_iter)
    return _REF[key]


# merge: both measures, (num, den) = (1, 2) and (1, 1), min_count 0 and 3, compact on and off
MERGE_LISTS = ("K3", "K12", "K65")
MERGE_RULES = [dict(measure=m, num=nu, den=de, min_count=mc) for m in (MR.OVER_MIN, MR.OVER_UNION) for nu, de in ((1, 2), (1, 1)) for mc in (0, 3)]
PLAIN = dict(measure=MR.OVER_MIN, num=1, den=2, min_count=0)


def merge_lists(name):
    return MERGE_LISTS + (("near",) if name in BIG_FRAMES else ())


def merge_ref(pkg, O, name, which, rule=None, compact=False, masked=False):
    """-> (records, parent, overlap, count) of merge_ref.merge on the frame under the frame's own score mode"""
    rule = PLAIN if rule is None else rule
    key = ("merge", name, which, tuple(sorted(rule.items())), compact, masked)
    if key not in _REF:
        src, tgt, kw, mode, frame = P.frame_case(pkg, O, name)
        rt, st = frame_lists(pkg, O, name)[which]
        with np.errstate(all="ignore"):
            _REF[key] = MR.merge(O, src, tgt, rt, kw["tau"], P.third_off(len(src)) if masked else None, st, mode, compact=compact, **rule)
    return _REF[key]


# ================================================================================================================================
# shapes at unit scale: past one trip of the overlap launch's word loop and of the settle deal; the decide launch's rounds
# ================================================================================================================================
SHAPE_NS = (2048, 2049, 2113)
SHAPE_K_MERGE, SHAPE_K_SETTLE = 33, 8
DECIDE_N = 129
DECIDE_KS = (65, 127, 128, 129, 130)
TIE_K, TIE_COPIES = 130, 72
# the copies' numbers: the original at 60, copies from 3 on below it and from 61 on above it — tied ranks 0 .. 72 of the strength
# order: they fill the first round's last ranks and reach into the second
TIE_AT, TIE_BELOW = 60, tuple(range(3, 33))
TIE_ABOVE = tuple(range(61, 61 + TIE_COPIES - len(TIE_BELOW)))


def shape_scene(pkg, n):
    return MR.scene(pkg, n)


SHAPE_SEED = 7


def shape_poses(pkg, n, K):
    sc = shape_scene(pkg, n)
    return MR.many(MR.rt_of(sc.R_gt, sc.t_gt), K, SHAPE_SEED)


def shape_frame(pkg, O, n, score_mode=0):
    """-> (kw, frame): the restatement's whole path on the shape scene under merge_ref.kw_of(), once per session"""
    key = ("shape frame", n, score_mode)
    if key not in _REF:
        sc = shape_scene(pkg, n)
        kw = MR.kw_of()
        _REF[key] = (kw, O.register(sc.src, sc.tgt, threads=min(O.max_threads(), 8), score_mode=score_mode, **kw))
    return _REF[key]


def shape_merge_ref(pkg, O, n, rule=None, compact=False):
    rule = PLAIN if rule is None else rule
    key = ("shape merge", n, tuple(sorted(rule.items())), compact)
    if key not in _REF:
        sc = shape_scene(pkg, n)
        _REF[key] = MR.merge(O, sc.src, sc.tgt, shape_poses(pkg, n, SHAPE_K_MERGE), MR.TAU, compact=compact, **rule)
    return _REF[key]


def shape_settle_ref(pkg, O, n, score_mode=0, max_iter=16):
    key = ("shape settle", n, score_mode, max_iter)
    if key not in _REF:
        sc = shape_scene(pkg, n)
        _REF[key] = SR.settle(O, sc.src, sc.tgt, shape_poses(pkg, n, SHAPE_K_SETTLE), SR.TAU, score_mode=score_mode, max_iter=max_iter)
    return _REF[key]


def decide_poses(pkg, O, K):
    """K poses on the n = 129 frame: merge_ref.many's; K = TIE_K: with TIE_COPIES exact copies of the list's strongest pose"""
    key = ("decide poses", K)
    if key not in _REF:
        sc = shape_scene(pkg, DECIDE_N)
        poses = MR.many(MR.rt_of(sc.R_gt, sc.t_gt), K, 100 + DECIDE_N + K)
        if K == TIE_K:
            score = MR.support(O, sc.src, sc.tgt, poses, MR.TAU)[3]
            best = poses[MR.strength_order(score)[0]].copy()
            poses[list(TIE_BELOW) + [TIE_AT] + list(TIE_ABOVE)] = best
        _REF[key] = poses
    return _REF[key]


def decide_ref(pkg, O, K, rule=None, compact=False):
    rule = PLAIN if rule is None else rule
    key = ("decide", K, tuple(sorted(rule.items())), compact)
    if key not in _REF:
        sc = shape_scene(pkg, DECIDE_N)
        _REF[key] = MR.merge(O, sc.src, sc.tgt, decide_poses(pkg, O, K), MR.TAU, compact=compact, **rule)
    return _REF[key]


def nothing_kept_rule(pkg, O, K):
    """a min_count above every count of the K-list"""
    return dict(PLAIN, min_count=int(decide_ref(pkg, O, K)[0]["count"].max()) + 1)


# ================================================================================================================================
# batches
# ================================================================================================================================
BATCH_NAMES, BATCH_LAUNCHES = P.ASSIGN_BATCH_NAMES, P.ASSIGN_LAUNCHES
SETTLE_BATCH_KS = (1, 3, SETTLE_BATCH_MAX_POSES)
SETTLE_BATCH_RUNS = [(K, 16) for K in SETTLE_BATCH_KS] + [(SETTLE_BATCH_MAX_POSES, 2)]   # (K, max_iter); 2: SC_POLISH_STOP_MAX_ITER
MERGE_BATCH_KS = (1, 3, 16, 64)
MERGE_BATCH_RULES = [dict(PLAIN), dict(measure=MR.OVER_UNION, num=1, den=1, min_count=3)]


def batch_problem(pkg, O, name, K):
    """-> (src, tgt, kw, Rt (K, 12), statuses (K,)) of one batch problem"""
    src, tgt, kw, _, _ = TR.polish_case(pkg, O, name, "winner", TR.MAX_ITER)
    rt, st = P.assign_batch_poses(pkg, O, name)[K]
    return src, tgt, kw, rt, st


def batch_input(pkg, O, gid, K):
    """-> (kw, problems, pose Rt (K, B, 12), statuses (K, B)) of one launch"""
    kw, names = BATCH_LAUNCHES[gid]
    per = [batch_problem(pkg, O, name, K) for name in names]
    return kw, [(p[0], p[1]) for p in per], np.stack([p[3] for p in per], axis=1), np.stack([p[4] for p in per], axis=1)


def settle_batch_ref(pkg, O, gid, K, max_iter=16):
    key = ("settle batch", gid, K, max_iter)
    if key not in _REF:
        kw, problems, rt, st = batch_input(pkg, O, gid, K)
        with np.errstate(all="ignore"):
            _REF[key] = SR.batch(O, problems, rt, kw["tau"], st, 0, max_iter)
    return _REF[key]


def merge_batch_ref(pkg, O, gid, K, rule=None, compact=False):
    rule = PLAIN if rule is None else rule
    key = ("merge batch", gid, K, tuple(sorted(rule.items())), compact)
    if key not in _REF:
        kw, problems, rt, st = batch_input(pkg, O, gid, K)
        with np.errstate(all="ignore"):
            _REF[key] = MR.batch(O, problems, rt, kw["tau"], st, 0, compact=compact, **rule)
    return _REF[key]


def launch_of(name):
    """the launch a batch problem travels in, and its place there"""
    for gid, (_, names) in BATCH_LAUNCHES.items():
        if name in names:
            return gid, names.index(name)
    raise KeyError(name)


# ================================================================================================================================
# what the references say about the frames
# ================================================================================================================================
def scaling_rows(which, K):
    """the rows of a list whose pose scales with its frame (the hostile poses and the status records are the same at every k)"""
    if which == "K12":
        return [P.POLISH_POSES.index(p) for p in P.METAMORPHIC_POSES]
    fixed = set(P.ASSIGN_HOSTILE) | set(P.ASSIGN_STATUS) if which in ("K64", "K65") else set()
    return [k for k in range(K) if k not in fixed]


def _labelled(lab):
    return int((lab >= 0).sum())


def _moved(rec):
    return sorted(int(x) for x in rec["iters"] if x)


def _kept(res):
    rec, parent, x, count = res
    return parent == np.arange(len(parent))


def test_settle_on_the_frames_moves_poses_and_stops_in_both_ways(pkg, O):
    """Family a in window (n = 300): the rounds words of K12 at max_iter 1, 2, 16, what K12 and K64 label and move.  Over all frames:
    both stops, K64 at its sixteenth round on c:20:22 and f:tau25, poses that never moved, declined poses, all three statuses;
    f:tau25 labels every row; the byte mask switches every third row off."""
    stops, statuses, hows = set(), set(), set()
    for name in FRAME_CASES:
        if name in NO_FRAME:
            continue
        n = len(P.frame_case(pkg, O, name)[0])
        for part in settle_parts(name):
            for which, mi, masked in settle_runs(name, part):
                rec, lab, d2, rounds = settle_ref(pkg, O, name, which, mi, masked)
                print(name, which, mi, masked, "rounds", rounds.tolist(), "labelled", _labelled(lab), "moved", _moved(rec))
                ok = rec["status"] == SC_OK
                stops.add(int(rounds[1])); statuses |= {int(s) for s in rec["status"]}
                hows |= {(int(r["stop"]), int(r["iters"]) > 0) for r in rec[ok]}
                assert rounds[0] <= mi and (rounds[1] == MAX_ITER) == (rounds[0] == mi and bool((rec["stop"][ok] == MAX_ITER).any())), (name, which, mi)
                assert int(rec["iters"].max()) <= rounds[0] and (d2[lab < 0].view(np.uint32) == 0x7F800000).all(), (name, which, mi)
                if masked:
                    assert (lab[P.third_off(n) == 0] == -1).all(), (name, which)
        if name in COUNT_FRAMES or name in MODE_FRAMES:
            assert [settle_ref(pkg, O, name, "K12", mi)[3].tolist() for mi in P.MAX_ITERS] == [[1, MAX_ITER], [2, MAX_ITER], [10, FIXED]], name
            rec, lab, d2, rounds = settle_ref(pkg, O, name, "K12", 16)
            assert _labelled(lab) == 118 >= 100 and _moved(rec) == [9, 9, 9], name
            rec, lab, d2, rounds = settle_ref(pkg, O, name, "K64", 16)
            assert rounds.tolist() == [8, FIXED] and _labelled(lab) == 120 >= 100 and len(_moved(rec)) == 11, name
            assert _labelled(settle_ref(pkg, O, name, "K3", 16)[1]) >= 100, name
            part = settle_ref(pkg, O, name, "K64", 16, True)[1]
            assert 60 <= _labelled(part) < 120, name
    assert stops == {FIXED, MAX_ITER}
    for name in ("c:20:22", "f:tau25"):
        assert settle_ref(pkg, O, name, "K64", 16)[3].tolist() == [16, MAX_ITER], name
    assert {(FIXED, True), (DECLINED, False), (DECLINED, True), (MAX_ITER, True)} <= hows, hows   # (iters == 0: the declined poses)
    assert statuses == {SC_OK, SC_EINVAL, SC_ENOHYP}
    with np.errstate(all="ignore"):
        assert np.isinf(AR.tau2_of(P.frame_case(pkg, O, "f:tau25")[2]["tau"]))
    for which in ("K3", "K12", "K64"):
        assert (settle_ref(pkg, O, "f:tau25", which, 16)[1] >= 0).all(), which        # tau^2 = +inf: every one of the 300 rows
    # the mode1 / mode2 frames go through settle_scores: the tallies are not the member counts
    for name in MODE_FRAMES:
        rec, lab, _, _ = settle_ref(pkg, O, name, "K64", 16)
        members = np.bincount(lab[lab >= 0], minlength=len(rec))
        live = members > 0
        assert live.sum() >= 3 and (rec["score"][live] != members[live]).all() and (rec["score0"][live] != rec["score"][live]).any(), name


def test_settle_on_the_big_frames(pkg, O):
    """n = 1500.  The winner of scene_big is its pure-translation block: 200 exact rows, so a refit over ANY three of them gives the
    block's motion, and a list of the winner's neighbours collapses onto one pose: K12 and K64 settle in one round (their neighbours
    turn about the origin and fit nothing), K3 in 2 .. 3 with one live pose.  The list `near` does better at k = 62 — five counted
    rounds, four poses moving in at least four of them — and at k = -56 no list tried (shifts of 0.2 .. 0.8 tau, turns of 0.005 ..
    0.05 radians about the inliers' centroid, 2 .. 8 of them, two seeds) runs past two rounds: there the refits of the first round
    give one and the same bits, and pose 0 takes every row in the second.  K3 stays for both."""
    for name in BIG_FRAMES:
        assert len(P.frame_case(pkg, O, name)[0]) == 1500
        for which in ("K12", "K64"):
            assert settle_ref(pkg, O, name, which, 16)[3].tolist() == [1, FIXED], (name, which)
        rec, lab, _, rounds = settle_ref(pkg, O, name, "K3", 16)
        assert 2 <= rounds[0] <= 3 and rounds[1] == FIXED and _labelled(lab) >= 200, name
        rec, lab, _, rounds = settle_ref(pkg, O, name, "near", 16)
        print(name, "near", rounds.tolist(), _moved(rec), _labelled(lab))
        assert len(rec) == len(NEAR_SHIFTS) + NEAR_TURNS and _labelled(lab) >= 200 and len(_moved(rec)) >= 2, name
        assert settle_ref(pkg, O, name, "near", 2)[3].tolist() == [2, MAX_ITER], name
    rec, lab, _, rounds = settle_ref(pkg, O, "big:62", "near", 16)
    assert rounds.tolist() == [5, FIXED] and _moved(rec)[-4:] == [4, 5, 5, 5]      # >= 3 counted rounds, >= 2 poses moving in each
    assert settle_ref(pkg, O, "big:-56", "near", 16)[3].tolist() == [2, FIXED]


def test_merge_on_the_frames_folds_keeps_and_drops(pkg, O):
    for name in FRAME_CASES:
        if name in NO_FRAME:
            continue
        for which in merge_lists(name):
            for rule in MERGE_RULES:
                res = merge_ref(pkg, O, name, which, rule)
                rec, parent, x, count = res
                packed = merge_ref(pkg, O, name, which, rule, compact=True)
                kept = _kept(res)
                valid = parent >= 0 if rule["min_count"] == 0 else None
                assert count[0] == kept.sum() and np.array_equal(np.diag(x), rec["count"]) and np.array_equal(x, x.T), (name, which, rule)
                assert np.array_equal(packed[1], parent) and np.array_equal(packed[2], x) and packed[3].tolist() == count.tolist()
                assert packed[0].tobytes() == np.concatenate([rec[kept], rec[~kept]]).tobytes(), (name, which, rule)
                if valid is not None:
                    assert count[1] == valid.sum(), (name, which)
            print(name, which, [merge_ref(pkg, O, name, which, rule)[3].tolist() for rule in MERGE_RULES])
    drop3 = dict(PLAIN, min_count=3)
    for name in COUNT_FRAMES + MODE_FRAMES:
        rec, parent, x, count = merge_ref(pkg, O, name, "K65")
        assert count.tolist() == [14, 61] and parent[5] == parent[1] != 5, name          # the exact copy never survives
        assert merge_ref(pkg, O, name, "K3")[3].tolist() == [1, 3], name
        # a valid pose with an empty support is the same as nothing (x >= 1 never holds): kept under min_count 0, dropped under 3
        empty = (rec["status"] == SC_OK) & (rec["count"] == 0) & (parent >= 0)
        assert int((_kept((rec, parent, x, count)) & (rec["count"] == 0)).sum()) == 13 == int(empty.sum()), name
        r3 = merge_ref(pkg, O, name, "K65", drop3)
        assert r3[3].tolist() == [1, 61] and not (_kept(r3) & (r3[0]["count"] < 3)).any() and (r3[1][rec["count"] < 3] == -1).all(), name
        tight = merge_ref(pkg, O, name, "K65", dict(measure=MR.OVER_UNION, num=1, den=1, min_count=0))
        assert tight[3][0] > count[0] and tight[1][5] == tight[1][1] != 5, name          # ... under the tightest rule either
    # the strength is the score: in the truncated modes the copy's parent is another pose than in the count mode
    assert {name: int(merge_ref(pkg, O, name, "K65")[1][5]) for name in COUNT_FRAMES} == {name: 1 for name in COUNT_FRAMES}
    for name in MODE_FRAMES:
        rec, parent, _, _ = merge_ref(pkg, O, name, "K65")
        assert int(parent[5]) == (64 if name.endswith("mode1") else 49), name
        assert MR.strength_order(rec["score"]) != MR.strength_order(rec["count"]), name
    # tau^2 = +inf: the finite poses all overlap fully
    rec, parent, x, count = merge_ref(pkg, O, "f:tau25", "K65")
    assert count.tolist() == [4, 61] and int(rec["count"].max()) == 300
    # the byte mask: a third of every support is gone
    full, part = merge_ref(pkg, O, "a:0", "K65")[0], merge_ref(pkg, O, "a:0", "K65", masked=True)[0]
    assert 0 < int(part["count"][P.WINNER_AT]) < int(full["count"][P.WINNER_AT])
    for name in BIG_FRAMES:
        assert merge_ref(pkg, O, name, "near")[3].tolist() == [1, len(NEAR_SHIFTS) + NEAR_TURNS] and merge_ref(pkg, O, name, "K65")[3].tolist() == [14, 61]


def test_inside_the_window_the_references_are_covariant(pkg, O):
    """What the GPU files' metamorphic checks rest on: at the k of polish_metamorphic_ks every integer of a settle or merge result is
    that at k = 0, R's bits too, t is multiplied by 2^k and d2 by 2^2k."""
    ks = R.polish_metamorphic_ks()
    assert len(ks) >= 3
    for k in ks:
        f = pow2(k)
        for which, mi, masked in SETTLE_RUNS:
            (rec, lab, d2, rounds), (rec0, lab0, d20, rounds0) = settle_ref(pkg, O, f"a:{k}", which, mi, masked), settle_ref(pkg, O, "a:0", which, mi, masked)
            rows = scaling_rows(which, len(rec))
            assert np.array_equal(lab, lab0) and rounds.tolist() == rounds0.tolist(), (k, which, mi)
            assert all(np.array_equal(rec[x], rec0[x]) for x in ("status", "score0", "score", "iters", "stop")), (k, which, mi)
            assert rec["Rt"][:, :9].tobytes() == rec0["Rt"][:, :9].tobytes(), (k, which, mi)
            assert rec["Rt"][rows][:, 9:].tobytes() == (rec0["Rt"][rows][:, 9:] * f).tobytes() and rec0["iters"][rows].any(), (k, which, mi)
            with np.errstate(all="ignore"):
                assert d2.tobytes() == np.where(lab0 >= 0, d20 * f * f, np.float32(np.inf)).astype(np.float32).tobytes(), (k, which, mi)
        for which in MERGE_LISTS:
            for rule in MERGE_RULES:
                for compact in (False, True):
                    m, m0 = merge_ref(pkg, O, f"a:{k}", which, rule, compact), merge_ref(pkg, O, "a:0", which, rule, compact)
                    assert_merge_covariant(m, m0, f, scaling_rows(which, len(m[0])), compact, (k, which, rule, compact))


def assert_merge_covariant(m, m0, f, rows, compact, what):
    """a merge result at scale f against the one at unit scale (the GPU file's metamorphic check runs it on the GPU's results)"""
    (rec, parent, x, count), (rec0, parent0, x0, count0) = m, m0
    assert all(np.array_equal(rec[c], rec0[c]) for c in ("status", "index", "count", "score")), what
    assert np.array_equal(parent, parent0) and np.array_equal(x, x0) and count.tolist() == count0.tolist(), what
    assert rec["Rt"][:, :9].tobytes() == rec0["Rt"][:, :9].tobytes(), what
    if compact:                                                       # the records' places are the kept poses', then the others'
        kept = parent0 == np.arange(len(parent0))
        place = np.concatenate([np.flatnonzero(kept), np.flatnonzero(~kept)])
        rows = [int(np.flatnonzero(place == k)[0]) for k in rows]
    assert rec["Rt"][rows][:, 9:].tobytes() == (rec0["Rt"][rows][:, 9:] * f).tobytes() and rec0["Rt"][rows][:, 9:].any(), what


# ================================================================================================================================
# what the references say about the shapes and the decide rounds
# ================================================================================================================================
def test_the_shapes_cross_the_trip_boundaries(pkg, O):
    """n = 2048: exactly 32 words; 2049: a second pass of the overlap launch's word loop that holds one word with one bit, a second
    trip of settle_label with one chunk of one row; 2113: 34 words, the last of them partial"""
    assert [(n + 63) // 64 for n in SHAPE_NS] == [32, 33, 34]
    assert all(shape_frame(pkg, O, n)[1]["rc"] == SC_OK for n in SHAPE_NS + (DECIDE_N,))
    stops = set()
    for n in SHAPE_NS:
        sc = shape_scene(pkg, n)
        rec, parent, x, count = shape_merge_ref(pkg, O, n)
        assert count.tolist() == [6, SHAPE_K_MERGE] and len(sc.src) == n
        inl = MR.support(O, sc.src, sc.tgt, shape_poses(pkg, n, SHAPE_K_MERGE), MR.TAU)[1]
        tail = inl[:, 2048:].astype(np.int64)
        if n == 2049:      # row 2048 is in no support: the second pass holds one word without a bit and 31 words past the row's end
            assert not tail.any()
        if n == 2113:      # 65 rows in the second pass, in the supports of several poses: what it adds is in the table
            assert (np.diag(tail @ tail.T) > 0).sum() >= 10 and (np.triu(tail @ tail.T, 1) > 0).sum() >= 10
        for mode in (0, 2):
            rec, lab, d2, rounds = shape_settle_ref(pkg, O, n, mode)
            print(n, mode, rounds.tolist(), _labelled(lab), rec["score"].tolist())
            stops.add(int(rounds[1]))
            if n == 2049:
                assert rounds.tolist() == [12, FIXED] and _labelled(lab) == 618, (n, mode)
            if n == 2113:
                assert rounds.tolist() == [16, MAX_ITER] and _labelled(lab) == 634 and (lab[2048:] >= 0).any(), (n, mode)
            members = np.bincount(lab[lab >= 0], minlength=SHAPE_K_SETTLE)
            assert np.array_equal(rec["score"] == members, np.full(SHAPE_K_SETTLE, mode == 0) | (members == 0)), (n, mode)
    assert stops == {FIXED, MAX_ITER}


def test_the_decide_lists_cross_the_round_boundaries_and_tie_across_them(pkg, O):
    for K in DECIDE_KS:
        rec, parent, x, count = decide_ref(pkg, O, K)
        print(K, count.tolist())
        assert count[1] == K and 2 <= count[0] < K and (parent >= 0).all()
        order = MR.strength_order(rec["score"])
        late = [k for k in order[64:] if parent[k] != k]
        print(K, "folded after the first round", len(late), "rank 64:", order[64], int(parent[order[64]]))
        if K > 65:         # a later round folds into a pose kept in the first (K = 65: the one rank of round two is a far pose, kept)
            assert late and any(order.index(int(parent[k])) < 64 for k in late), K
        # min_count above every count: nothing is kept, nothing is folded, and compact leaves the order ascending
        rule = nothing_kept_rule(pkg, O, K)
        for compact in (False, True):
            none = decide_ref(pkg, O, K, rule, compact)
            assert none[3].tolist() == [0, K] and (none[1] == -1).all() and (none[0]["status"] == SC_ENOHYP).all(), K
            assert np.array_equal(none[0]["count"], rec["count"]) and np.array_equal(none[0]["index"], np.full(K, -1)), K
            assert none[0].tobytes() == decide_ref(pkg, O, K, rule, False)[0].tobytes(), K    # compact: nothing moves, the order stays ascending
    # the ties: the strongest pose and its 72 copies hold the ranks 0 .. 72 in the order of their numbers
    rec, parent, x, count = decide_ref(pkg, O, TIE_K)
    tied = sorted(TIE_BELOW + (TIE_AT,) + TIE_ABOVE)
    order = MR.strength_order(rec["score"])
    assert len(tied) - 1 == TIE_COPIES >= 70 and order[:len(tied)] == tied and min(tied) < TIE_AT < max(tied)
    assert order.index(TIE_AT) < 63 and len(tied) > 64                # the tied ranks straddle rank 63 | 64
    assert (parent[tied] == tied[0]).all() and rec[tied[0]]["status"] == SC_OK and (rec["status"][tied[1:]] == SC_ENOHYP).all()
    assert len(np.unique(rec["score"][tied])) == 1 and int(rec["score"][tied[0]]) == int(rec["score"].max())


# ================================================================================================================================
# what the references say about the batches
# ================================================================================================================================
def _near(name, K, st, rt):
    """the valid poses of assign_batch_poses' K-list that are neighbours of the winner: not assign_ref.many's far ones, not hostile"""
    return [k for k in range(K) if st[k] == SC_OK and np.isfinite(rt[k]).all() and (K == 3 or (k % 7 != 3 and k not in P.BATCH_HOSTILE))]


def test_the_batches_underflow_overflow_and_stay_small(pkg, O):
    assert all(len(names) <= 40 for _, names in BATCH_LAUNCHES.values()) and sum(len(n) for _, n in BATCH_LAUNCHES.values()) == len(BATCH_NAMES)
    assert max(len(TR.polish_case(pkg, O, name)[0]) for name in BATCH_NAMES) <= 512
    assert SETTLE_BATCH_KS == (1, 3, 16) and MERGE_BATCH_KS == (1, 3, 16, 64)
    stops = set()
    for gid in BATCH_LAUNCHES:
        for K, mi in SETTLE_BATCH_RUNS:
            rec, labels, rounds = settle_batch_ref(pkg, O, gid, K, mi)
            stops |= set(rounds[:, 1].tolist())
            print(gid, "settle", K, mi, rounds.tolist(), [_labelled(l) for l in labels])
        for K in MERGE_BATCH_KS:
            for rule in MERGE_BATCH_RULES:
                rec, parent, count = merge_batch_ref(pkg, O, gid, K, rule)
                packed = merge_batch_ref(pkg, O, gid, K, rule, compact=True)
                assert np.array_equal(packed[1], parent) and np.array_equal(packed[2], count), (gid, K)
            print(gid, "merge", K, merge_batch_ref(pkg, O, gid, K)[2].tolist())
    assert {FIXED, MAX_ITER} <= stops
    # a:*:-70: tau^2 is the smallest subnormal, so a support row is a row whose residual is exactly 0; the near poses' residuals on
    # the rows any of them holds are 0, one or two subnormal steps, and which of the three a row gets differs from pose to pose.  So
    # the supports are NOT one set and the scores do not all tie (n = 192, K = 3: 37, 39, 37 rows) — but they overlap by far more than
    # half, and in the count mode exactly one near pose is kept: the strongest, and among the strongest the lowest-numbered.
    for n in R.SCENES:
        name = f"a:{n}:-70"
        gid, b = launch_of(name)
        for K in (3, 16, 64):
            src, tgt, kw, rt, st = batch_problem(pkg, O, name, K)
            with np.errstate(all="ignore"):
                tau2 = AR.tau2_of(kw["tau"])
                status, inl, cnt, score = MR.support(O, src, tgt, rt, kw["tau"], None, st)
            near = _near(name, K, st, rt)
            with np.errstate(all="ignore"):
                D = AR.resid2(rt[near], src, tgt)
            assert tau2 == np.float32(2.0 ** -149) and len(near) >= min(K, 3)
            held = inl[near].any(axis=0)
            assert np.array_equal(inl[near], D == 0) and (cnt[near] >= 30).all() and (D[:, held] <= np.float32(2.0 ** -148)).all(), (name, K)
            assert np.array_equal(score[near], cnt[near]) and len(set(cnt[near].tolist())) > 1, (name, K)
            rec, parent, count = merge_batch_ref(pkg, O, gid, K)
            first = min(k for k in near if cnt[k] == cnt[near].max())
            assert [k for k in near if parent[k, b] == k] == [first] and (parent[near, b] == first).all(), (name, K)
            srec, labels, rounds = settle_batch_ref(pkg, O, gid, min(K, SETTLE_BATCH_MAX_POSES))
            assert _labelled(labels[b]) >= 3, (name, K)
    # a:*:70 and e: a row with a non-finite residual is in no support and gets the label -1
    for name in [f"a:{n}:70" for n in R.SCENES] + ["e"]:
        gid, b = launch_of(name)
        for K in (3, 16):
            src, tgt, kw, rt, st = batch_problem(pkg, O, name, K)
            valid = [k for k in range(K) if st[k] == SC_OK and np.isfinite(rt[k]).all()]
            with np.errstate(all="ignore"):
                bad = ~np.isfinite(AR.resid2(rt[valid], src, tgt))
                inl = MR.support(O, src, tgt, rt, kw["tau"], None, st)[1]
            srec, labels, rounds = settle_batch_ref(pkg, O, gid, K)
            assert bad.any() and not inl[valid][bad].any() and (labels[b][bad.all(axis=0)] == -1).all(), (name, K)
            if name == "e":      # the rows whose target is at +-3e38 (the zero pose takes the source row 10 to the origin); the others are labelled
                assert bad.all(axis=0)[[11, 70, 90]].all() and _labelled(labels[b]) >= 50 and 3 <= bad.all(axis=0).sum() < 10, K
            else:
                assert bad.all() and (labels[b] == -1).all() and rounds[b].tolist() == [0, FIXED], (name, K)
    # in window the counted rounds are not zero: the starts are no fixed points
    for name in ("a:300:0", "a:512:62", "a:192:-56"):
        gid, b = launch_of(name)
        assert settle_batch_ref(pkg, O, gid, 16)[2][b, 0] >= 3 and merge_batch_ref(pkg, O, gid, 64)[2][b].tolist() == [14, 60], name
