"""CPU suite: the inputs of tests/test_gpu_pose_frame_range.py, tests/test_gpu_pose_batch_range.py and
tests/test_gpu_match_guided_range.py — sc_polish_poses, sc_pose_info_frame, sc_assign_poses (frame and batch), sc_pose_info_batch
(plain, slot and pairs forms) and the guided matchers at the ends of the fp32 range — and what the REFERENCES alone say about them.

The three GPU files compare the kernels with tests/polish_poses_ref.py, pose_info_frame_ref.py, pose_info_ref.py, assign_ref.py,
match_guided_ref.py, match_guided_batch_ref.py and match_guided_poses_ref.py bit for bit.  That is only worth something if the
inputs leave the beaten path for the reason meant (residuals that underflow to 0, tau^2 = +inf, every stop of a refit, gates whose
square is 0 or +inf, whole tiles that no pose admits), and if the emulated fma every residual bit hangs on is right out there.  All of
that is asserted here, on the references alone.  This file owns the case tables and the helpers that build the inputs and the
reference results (once per session, never modified); scenes, families and parameter tables are those of tests/test_range_oracle.py,
tests/test_batch_range_ref.py and tests/test_batch_tail_range_ref.py (imported, not copied).

Frames (sc_polish_poses, sc_pose_info_frame, sc_assign_poses on a frame): test_batch_range_ref.polish_input on scene_small (n = 300)
— family a at POLISH_KS, c:20:22, e, f:tau-30, f:tau25, the mode1 / mode2 cases, sparse:+-40 — plus scene_big (n = 1500, 24 chunks)
at k = 62 and k = -56.  NO_FRAME names the cases whose reference frame is SC_ENOHYP: the only ones that may take the GPU file's
no-frame branch.  "In window" is test_range_oracle.WIN_C2: tau^2 and the squared residuals next to it are normal numbers.

Pose lists.  polish / pose-info: test_batch_tail_range_ref.pose_of on the frame's winner (POLISH_POSES) plus the winner under status
-1 and -5.  assign: assign_ref.perturbed / many on the winner with its translation taken back to unit scale (an exact division by
2^k), the results' translations times 2^k again, the hostile poses and the status records at fixed positions in between.

Condition "at least 100 correspondences labelled at n = 300": holds on every in-window frame (scene_small: the winner has 117
inliers).  The batch scene of n = 300 cannot meet it — 90 of its correspondences follow the motion at all, the winner keeps 85 —, so
for the batch the condition is asserted on the nearest scene that can, n = 512 (winner: 101), at every in-window k and K >= 3; at
n = 192 and 300 the floor is half the winner's own count (a neighbour a fraction of tau away keeps most of the winner's inliers).
The frames sparse:+-40 hold 500 correspondences (polish_ref.sparse_scene), the others 300 and 1500.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import assign_ref as AR
import batch_ref
import match_guided_batch_ref as GB
import match_guided_poses_ref as MP
import match_guided_ref as MG
import match_ref
import polish_poses_ref as PP
import pose_info_frame_ref as PIF
import pose_info_ref as PI
import test_batch_range_ref as R
import test_batch_tail_range_ref as TR
from test_range_oracle import UNIT, WIN_C2, in_window, pow2, scaled, scaled_kw, scene_big, translated

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
_QUIET = dict(over="ignore", under="ignore", divide="ignore", invalid="ignore")
_REF = {}


# ================================================================================================================================
# the emulated fma at the range ends
# ================================================================================================================================
def round_to_f32(x):
    """a rational, rounded once to fp32 (nearest, ties to even; subnormals; overflow to inf) -> np.float32"""
    if x == 0:
        return np.float32(0.0)
    sign, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()       # 2^(e-1) < a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1                                                       # 2^e <= a < 2^(e+1)
    q = max(e, -126) - 23                                            # the ulp's exponent (subnormals: fixed at -149)
    m = a / Fraction(2) ** q
    n = m.numerator // m.denominator
    rest = m - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    if n * Fraction(2) ** q >= Fraction(2) ** 128:
        return np.float32(sign * np.inf)
    return np.float32(sign * math.ldexp(n, q))                       # n < 2^25, q >= -149: exact in fp64, and representable in fp32


def fma_triples(count, seed=20):
    """seeded (a, b, c): operand exponents from 2^-80 to 2^70; the addend of random magnitude down to 2^-149 (a third of the
    triples), or within 2^-1 .. 2^-30 of cancelling the product (the rest)"""
    rng = np.random.default_rng(seed)

    def operand(lo, hi):
        m = (1 + rng.random(count)) * rng.choice([-1.0, 1.0], count)
        return (m * np.exp2(rng.integers(lo, hi + 1, count).astype(np.float64))).astype(np.float32)

    with np.errstate(**_QUIET):
        a, b = operand(-80, 70), operand(-80, 70)
        c = operand(-149, 127)
        prod = a.astype(np.float64) * b.astype(np.float64)
        near = (-prod * (1 + rng.choice([-1.0, 1.0], count) * np.exp2(-rng.integers(1, 31, count).astype(np.float64)))).astype(np.float32)
        cancel = rng.random(count) > 1 / 3
        c = np.where(cancel & np.isfinite(near), near, c).astype(np.float32)
    return a, b, c


def test_the_emulated_fma_equals_exact_arithmetic_rounded_once():
    """assign_ref.fmaf against fractions.Fraction rounded once to fp32: subnormal results, results that round up into the normal
    range, cancellation to a few bits, and overflow.  Every residual bit of the three GPU files hangs on it."""
    a, b, c = fma_triples(24000)
    got = AR.fmaf(a, b, c)
    exp = np.array([round_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], np.float32)
    sub = (exp != 0) & (np.abs(exp) < np.float32(2.0 ** -126))
    print("triples", len(a), "subnormal results", int(sub.sum()), "zeros", int((exp == 0).sum()), "overflows", int(np.isinf(exp).sum()),
          "mismatches", int((got.view(np.uint32) != exp.view(np.uint32)).sum()))
    # (a product overflows where the two exponents, uniform on -80 .. 70, sum to 127 or more: 91 of 151^2 pairs, about 96 triples)
    assert sub.sum() > 200 and np.isinf(exp).sum() > 50 and (exp == 0).sum() > 20
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    # the rounding helper itself, on values whose fp32 neighbour is known
    f = np.float32
    assert round_to_f32(Fraction(1) + Fraction(1, 2 ** 24)) == f(1) and round_to_f32(Fraction(1) + Fraction(3, 2 ** 24)) == f(1 + 2.0 ** -22)
    assert round_to_f32(Fraction(1, 2 ** 150)) == f(0) and round_to_f32(Fraction(3, 2 ** 150)) == f(2.0 ** -148)
    assert round_to_f32(Fraction(2) ** 128 - Fraction(2) ** 103) == f(np.inf) and round_to_f32(-(Fraction(2) ** 128 - Fraction(2) ** 104)) == -np.finfo(f).max


# ================================================================================================================================
# frames: sc_polish_poses, sc_pose_info_frame, sc_assign_poses on a frame
# ================================================================================================================================
FRAME_CASES = list(R.POLISH_CASES) + ["big:62", "big:-56"]
NO_FRAME = ("f:tau-30",)                       # the reference frame is SC_ENOHYP: the three entries refuse with SC_EINVAL
POLISH_POSES = ("winner", "shift:0.5", "shift:0.9", "shift:1.5", "shift:3.0", "t3e38", "R3e38", "zero", "nan", "inf")
POLISH_STATUSES = (SC_EINVAL, SC_ENOHYP)       # the winner's pose under these statuses, behind the ten
MAX_ITERS = (1, 2, 16)
SEL_FRAME = "a:62"                             # the frame SEL_LABEL / SEL_ALIVE run on
METAMORPHIC_POSES = ("winner", "shift:0.5", "shift:0.9", "shift:1.5", "shift:3.0")
ASSIGN_LISTS = ("K3", "K65")
ASSIGN_SEED = 953                              # one seed for every frame (test_assign_on_the_frames_discriminates: it discriminates on each)
# K65: assign_ref.many(65) with these positions replaced (none of them is the copy at 5, its original at 1 or a far pose at 3 + 7 i)
ASSIGN_HOSTILE = {9: "t3e38", 20: "R3e38", 30: "zero", 40: "hostile", 50: "nan", 60: "inf"}
ASSIGN_STATUS = {12: SC_EINVAL, 22: SC_ENOHYP}  # good poses under a status that switches them off
WINNER_AT = 14                                  # ... and the winner itself (far from the origin its neighbours fit nothing: they turn about the origin)


def frame_k(name):
    fam, *arg = name.split(":")
    return int(arg[0]) if fam in ("a", "sparse", "big") else 0


def frame_in_window(name):
    return name.split(":")[0] in ("a", "big") and in_window(frame_k(name), WIN_C2)


IN_WINDOW_FRAMES = [name for name in FRAME_CASES if frame_in_window(name)]


def frame_case(pkg, O, name):
    """-> (src, tgt, kw, score_mode, frame): the restatement's whole path on the case, once per session"""
    if not name.startswith("big:"):
        return R.polish_case_ref(pkg, O, name)[:5]
    if ("frame", name) not in _REF:
        k = frame_k(name)
        src, tgt = scene_big(pkg)
        src, tgt, kw = scaled(src, k), scaled(tgt, k), dict(scaled_kw(k), max_triangles=R.POLISH_T)
        with np.errstate(**_QUIET):
            frame = O.register(src, tgt, threads=min(O.max_threads(), 8), score_mode=0, **kw)
        _REF["frame", name] = (src, tgt, kw, 0, frame)
    return _REF["frame", name]


def winner_of(frame):
    return np.concatenate([np.asarray(frame["R"], np.float32).ravel(), np.asarray(frame["t"], np.float32)]).astype(np.float32)


def third_off(n):
    """the byte mask of the SEL_MASK runs: every third row switched off"""
    return (np.arange(n) % 3 != 0).astype(np.uint8)


def crafted_label(n):
    """the label array of the SEL_LABEL / SEL_ALIVE runs: -1 .. 12 in turn, so that each of the twelve records owns some rows"""
    return (np.arange(n) % 14 - 1).astype(np.int32)


def frame_poses(pkg, O, name):
    """-> (Rt (12, 12) float32, statuses (12,) int32): POLISH_POSES of the frame's winner, then the winner under POLISH_STATUSES"""
    src, tgt, kw, mode, frame = frame_case(pkg, O, name)
    w = winner_of(frame)
    rt = np.stack([TR.pose_of(w, kw["tau"], p) for p in POLISH_POSES] + [w] * len(POLISH_STATUSES))
    return rt, np.array([SC_OK] * len(POLISH_POSES) + list(POLISH_STATUSES), np.int32)


def records64(rt, statuses):
    """pose records of 64 bytes (sc_polish_batch_result's head): Rt, the status at byte 48, a pattern behind it"""
    rec = np.frombuffer(bytes([0xA5]) * (64 * len(rt)), GB.POSE64).copy()
    rec["Rt"], rec["status"] = rt, statuses
    return rec


def _sel_of(n, sel_mode):
    return None if sel_mode == PP.SEL_NONE else third_off(n) if sel_mode == PP.SEL_MASK else crafted_label(n)


def polish_ref(pkg, O, name, max_iter, sel_mode=PP.SEL_NONE, with_status=True):
    """-> (records, masks) of polish_poses_ref.poses on the frame's twelve records (with_status False: the ten poses, nothing read
    behind byte 47)"""
    key = ("polish", name, max_iter, sel_mode, with_status)
    if key not in _REF:
        src, tgt, kw, mode, frame = frame_case(pkg, O, name)
        rt, st = frame_poses(pkg, O, name)
        if not with_status:
            rt, st = rt[:len(POLISH_POSES)], None
        with np.errstate(**_QUIET):
            _REF[key] = PP.poses(O, src, tgt, rt, kw["tau"], sel_mode, _sel_of(len(src), sel_mode), statuses=st, score_mode=mode, max_iter=max_iter)
    return _REF[key]


def info_poses(pkg, O, name, which):
    """the pose records of a pose-info call: "in": the twelve input records; "polished": the reference's polished records of the
    max_iter 16, SEL_NONE call (64 bytes each, their own statuses)"""
    if which == "in":
        return records64(*frame_poses(pkg, O, name))
    return polish_ref(pkg, O, name, 16)[0].copy()


def info_ref(pkg, O, name, which, sel_mode=PIF.SEL_NONE):
    key = ("info", name, which, sel_mode)
    if key not in _REF:
        src, tgt, kw, mode, frame = frame_case(pkg, O, name)
        rec = info_poses(pkg, O, name, which)
        with np.errstate(**_QUIET):
            _REF[key] = PIF.frame(O, src, tgt, rec["Rt"], kw["tau"], sel_mode, _sel_of(len(src), sel_mode), statuses=rec["status"])
    return _REF[key]


def pose_lists(winner, k, tau, seed, sizes=(3, 65), hostile=ASSIGN_HOSTILE, status=ASSIGN_STATUS):
    """the pose lists of sc_assign_poses around `winner` of a scene at scale 2^k -> {K: (Rt (K, 12), statuses (K,))}.
    K = 1: the winner; K = 3: two neighbours and a copy of the first; larger: assign_ref.many with the hostile poses and the status
    records at the positions given (those beyond K dropped) and the winner itself at WINNER_AT."""
    base = np.array(winner, np.float32)
    base[9:] = scaled(base[9:], -k)                                  # exact: a power of two, and |t| is far from both ends
    out = {}
    for K in sizes:
        st = np.zeros(K, np.int32)
        if K == 1:
            rt = base[None, :].copy()
        elif K == 3:
            two = AR.perturbed(base, 2, seed)
            rt = np.stack([two[0], two[1], two[0]])
        else:
            rt = AR.many(base, K, seed + K)
        rt[:, 9:] = scaled(rt[:, 9:], k)
        if K > 3:
            big = np.array(winner, np.float32)
            for pos, what in hostile.items():
                if pos < K:
                    rt[pos] = AR.hostile() if what == "hostile" else TR.pose_of(big, tau, what)
            for pos, s in status.items():
                if pos < K:
                    st[pos] = s
            rt[WINNER_AT] = big
        out[K] = (np.ascontiguousarray(rt, np.float32), st)
    return out


def assign_poses(pkg, O, name):
    """-> {"K3": (Rt, None), "K65": (Rt, statuses)}: K3 goes in as bare floats (stride 48), K65 as records under SC_ASSIGN_STATUS"""
    key = ("assign poses", name)
    if key not in _REF:
        src, tgt, kw, mode, frame = frame_case(pkg, O, name)
        lists = pose_lists(winner_of(frame), frame_k(name), kw["tau"], ASSIGN_SEED)
        _REF[key] = {"K3": (lists[3][0], None), "K65": lists[65]}
    return _REF[key]


def assign_ref(pkg, O, name, which, mode, sel_mode=AR.SEL_NONE):
    """-> (label, d2, records) of assign_ref.assign on the frame"""
    key = ("assign", name, which, mode, sel_mode)
    if key not in _REF:
        src, tgt, kw, smode, frame = frame_case(pkg, O, name)
        rt, st = assign_poses(pkg, O, name)[which]
        with np.errstate(all="ignore"):
            _REF[key] = AR.assign(O, src, tgt, rt, kw["tau"], mode, None if sel_mode == AR.SEL_NONE else third_off(len(src)), st, smode)
    return _REF[key]


def test_the_frames_are_what_they_are_used_for(pkg, O):
    """Which frames exist (NO_FRAME names exactly the others), their sizes, and the winners the pose lists are built on."""
    none = []
    for name in FRAME_CASES:
        src, tgt, kw, mode, frame = frame_case(pkg, O, name)
        print(name, "n", len(src), "rc", frame["rc"], "count", frame["best_count"], "mode", mode)
        assert len(src) in (300, 500, 1500), name
        if frame["rc"] != SC_OK:
            none.append(name)
            assert frame["rc"] == SC_ENOHYP, name
        else:
            assert np.isfinite(winner_of(frame)).all(), name
    assert tuple(none) == NO_FRAME
    assert [len(frame_case(pkg, O, n)[0]) for n in ("big:62", "big:-56")] == [1500, 1500]
    assert {"a:0", "a:-56", "a:62", "big:62", "big:-56", "a:-56:mode1", "a:62:mode2"} <= set(IN_WINDOW_FRAMES) and "a:64" not in IN_WINDOW_FRAMES


def test_the_polish_poses_stop_in_every_way(pkg, O):
    """Over the frame cases at max_iter 1, 2, 16 under SEL_NONE: STOP_FIXED, STOP_DECLINED before the first refit and after one,
    STOP_MAX_ITER, every status, and shift:3.0 keeps no inlier."""
    hows, statuses = set(), set()
    shift3 = POLISH_POSES.index("shift:3.0")
    for name in FRAME_CASES:
        if name in NO_FRAME:
            continue
        for mi in MAX_ITERS:
            rec, masks = polish_ref(pkg, O, name, mi)
            hows |= {(int(r["stop"]), int(r["iters"]) > 0) for r in rec if r["status"] == SC_OK}
            statuses |= {int(s) for s in rec["status"]}
            assert rec["status"].tolist() == [SC_OK] * 8 + [SC_EINVAL, SC_EINVAL, SC_EINVAL, SC_ENOHYP], name
            for r in rec[8:]:                                        # nan, inf, and the two statuses: the identity, nothing kept
                assert r["Rt"].tobytes() == PP.IDENT.tobytes() and int(r["stop"]) == PP.STOP_DECLINED and not r["score"], name
            assert not masks[8:].any(), name
            if frame_in_window(name):                                # |shift| = 3 tau: no correspondence of the winner's stays within tau
                assert int(rec[shift3]["score0"]) == 0 and not masks[shift3].any() and int(rec[shift3]["stop"]) == PP.STOP_DECLINED, (name, mi)
        print(name, [(int(r["status"]), int(r["score0"]), int(r["score"]), int(r["iters"]), int(r["stop"])) for r in polish_ref(pkg, O, name, 16)[0]])
    assert {(PP.STOP_FIXED, True), (PP.STOP_DECLINED, False), (PP.STOP_DECLINED, True), (PP.STOP_MAX_ITER, True)} <= hows, hows
    assert statuses == {SC_OK, SC_EINVAL, SC_ENOHYP}
    # the selections change what a record sees: under the byte mask a third of the winner's inliers are gone
    for name in ("a:0", "big:-56"):
        full, part = polish_ref(pkg, O, name, 16)[0][0], polish_ref(pkg, O, name, 16, PP.SEL_MASK)[0][0]
        assert 0 < int(part["score0"]) < int(full["score0"]), name
    lab = polish_ref(pkg, O, SEL_FRAME, 16, PP.SEL_LABEL)[0]
    alive = polish_ref(pkg, O, SEL_FRAME, 16, PP.SEL_ALIVE)[0]
    assert lab.tobytes() != alive.tobytes() and int(alive[0]["score0"]) > int(lab[0]["score0"])


def test_the_pose_info_cases_hold_inliers_and_scale(pkg, O):
    """Every in-window frame: the winner's record has inliers and a non-zero sse; between k = 0 and k != 0 the scaled blocks differ
    (so the GPU file's metamorphic check does not compare zeros) and are exact multiples."""
    for name in IN_WINDOW_FRAMES:
        if name.startswith("big") or name.count(":") > 1:
            continue                                                 # (their winners' records are asserted on the GPU file's path)
        rec = info_ref(pkg, O, name, "in")[0]
        assert int(rec["status"]) == SC_OK and int(rec["inliers"]) > 0 and float(rec["sse"]) > 0, name
    r0 = info_ref(pkg, O, "a:0", "in")[0]
    i0 = r0["info"].reshape(6, 6)
    for k in R.polish_metamorphic_ks():
        r = info_ref(pkg, O, f"a:{k}", "in")[0]
        i, f = r["info"].reshape(6, 6), 2.0 ** k
        assert int(r["inliers"]) == int(r0["inliers"]) and float(r["sse"]) == float(r0["sse"]) * f * f != float(r0["sse"]), k
        assert np.array_equal(i[3:, 3:], i0[3:, 3:]) and np.array_equal(i[:3, 3:], i0[:3, 3:] * f) and np.array_equal(i[:3, :3], i0[:3, :3] * f * f), k
        assert not np.array_equal(i[:3, :3], i0[:3, :3]) and i0[:3, :3].any() and i0[:3, 3:].any(), k


def _labelled(lab):
    return int((lab >= 0).sum())


def test_assign_on_the_frames_discriminates(pkg, O):
    """In window, both lists: at least 100 correspondences labelled (n = 300), BEST and FIRST differ, the duplicate claims nothing.
    f:tau25: tau^2 = +inf and every row is labelled.  Outside the window the reference still defines the result (printed)."""
    for name in FRAME_CASES:
        if name in NO_FRAME:
            continue
        for which, dup in (("K3", 2), ("K65", 5)):
            (lb, db, rb), (lf, df, rf) = (assign_ref(pkg, O, name, which, m) for m in (AR.BEST, AR.FIRST))
            print(name, which, "labelled", _labelled(lb), "BEST != FIRST on", int((lb != lf).sum()), "dup", int(rb["count"][dup]), int(rf["count"][dup]))
            if frame_in_window(name):
                assert _labelled(lb) >= 100 and (lb != lf).any(), (name, which)
                assert int(rb["count"][dup]) == 0 == int(rf["count"][dup]), (name, which)
            if which == "K65":
                assert rb["status"][sorted(ASSIGN_HOSTILE)].tolist() == [SC_OK] * 4 + [SC_EINVAL] * 2
                assert rb["status"][sorted(ASSIGN_STATUS)].tolist() == [SC_EINVAL, SC_ENOHYP]
                assert not rb["count"][sorted(ASSIGN_STATUS) + [50, 60]].any(), name          # switched off or non-finite: nothing
                if frame_in_window(name):                            # (under tau^2 = +inf a finite hostile pose does claim rows; the zero
                    assert not rb["count"][[9, 20, 40]].any(), name  # pose claims the target points within tau of the origin: scene_big has three)
    src, tgt, kw, mode, frame = frame_case(pkg, O, "f:tau25")
    with np.errstate(all="ignore"):
        assert np.isinf(AR.tau2_of(kw["tau"]))
    for which in ASSIGN_LISTS:
        lab, d2, rec = assign_ref(pkg, O, "f:tau25", which, AR.BEST)
        assert (lab >= 0).all() and np.isfinite(d2).all(), which
    part = assign_ref(pkg, O, "a:0", "K65", AR.BEST, AR.SEL_MASK)[0]
    assert (part[::3] == -1).all() and _labelled(part) >= 60
    for mode_name in ("a:-56:mode1", "a:-56:mode2", "a:62:mode1", "a:62:mode2"):    # the truncated scores are not the counts
        rec = assign_ref(pkg, O, mode_name, "K65", AR.BEST)[2]
        assert (rec["score"][rec["count"] > 0] != rec["count"][rec["count"] > 0]).any(), mode_name


def test_inside_the_window_the_references_are_covariant(pkg, O):
    """What the GPU file's metamorphic check rests on: at the k of polish_metamorphic_ks the polish records, the information records
    and the assignments of METAMORPHIC_POSES / the assign lists are those at k = 0, lengths times 2^k."""
    rows = [POLISH_POSES.index(p) for p in METAMORPHIC_POSES]
    ks = R.polish_metamorphic_ks()
    assert len(ks) >= 3
    for k in ks:
        f = pow2(k)
        (pol, masks), (pol0, masks0) = polish_ref(pkg, O, f"a:{k}", 16), polish_ref(pkg, O, "a:0", 16)
        assert all(np.array_equal(pol[x][rows], pol0[x][rows]) for x in ("status", "score0", "score", "iters", "stop")), k
        assert pol["Rt"][rows][:, :9].tobytes() == pol0["Rt"][rows][:, :9].tobytes() and np.array_equal(masks[rows], masks0[rows]), k
        assert pol["Rt"][rows][:, 9:].tobytes() == (pol0["Rt"][rows][:, 9:] * f).tobytes(), k
        info, info0 = info_ref(pkg, O, f"a:{k}", "in")[rows], info_ref(pkg, O, "a:0", "in")[rows]
        assert np.array_equal(info["inliers"], info0["inliers"]) and info["sse"].tobytes() == (info0["sse"] * float(f) * float(f)).tobytes(), k
        for which in ASSIGN_LISTS:
            for mode in (AR.BEST, AR.FIRST):
                (lab, d2, rec), (lab0, d20, rec0) = assign_ref(pkg, O, f"a:{k}", which, mode), assign_ref(pkg, O, "a:0", which, mode)
                assert np.array_equal(lab, lab0) and rec.tobytes() == rec0.tobytes(), (k, which, mode)
                with np.errstate(all="ignore"):
                    assert d2.tobytes() == np.where(lab0 >= 0, d20 * f * f, np.float32(np.inf)).astype(np.float32).tobytes(), (k, which, mode)


# ---- the resid2 pin, extended ------------------------------------------------------------------------------------------------------
def _pin(O, Rt, src, tgt, rows):
    """test_assign_abi's pin on the given rows: so_mask on ONE correspondence says 0 at tau2 = d2 and 1 at nextafter(d2) — where d2 is
    finite and below FLT_MAX; an infinite or NaN residual is never below any threshold -> the number of rows pinned"""
    import ctypes as C
    L = O.lib()
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    rt = np.ascontiguousarray(Rt, np.float32)
    with np.errstate(all="ignore"):
        d2 = AR.resid2(rt, src[rows], tgt[rows])
    done = 0
    for i, m in enumerate(rows):
        p, q = np.ascontiguousarray(src[m]), np.ascontiguousarray(tgt[m])
        up = np.nextafter(d2[i], np.float32(np.inf)) if np.isfinite(d2[i]) else np.float32(np.inf)
        out = np.zeros(2, np.uint8)
        for j, thr in enumerate((d2[i], up)):
            thr = np.float32(np.inf) if np.isnan(thr) else thr
            L.so_mask(p.ctypes.data_as(f32p), q.ctypes.data_as(f32p), 1, rt.ctypes.data_as(f32p), C.c_float(float(thr)), out[j:].ctypes.data_as(u8p))
        want = [0, 1] if np.isfinite(d2[i]) else [0, 0]
        assert out.tolist() == want, (m, d2[i], out.tolist())
        done += 1
    return done, d2


def test_the_emulated_residual_is_the_restatements_at_the_range_ends(pkg, O):
    """test_assign_abi.py's pin on the inputs of this file: family a at k = -70, -56, 62, 70 (residuals that are 0, subnormal, huge,
    infinite), family e (rows at +-3e38: infinite residuals) and c:20:22 (quantised coordinates: exact ties)."""
    checked = 0
    rng = np.random.default_rng(12)
    for name in ("a:300:-70", "a:300:-56", "a:300:62", "a:300:70", "e", "c:20:22"):
        src, tgt, kw, rec, _ = R.case_ref(pkg, O, name)
        k = batch_k(name)
        w = rec["Rt"] if rec["status"] == SC_OK else scaled_t(R.case_ref(pkg, O, "a:300:0")[3]["Rt"], k)
        lists = pose_lists(w, k, kw["tau"], 77, sizes=(3,))
        rows = np.unique(np.concatenate([rng.choice(len(src), 60, replace=False), [10, 11, 70, 90]]))
        kinds = set()
        for Rt in list(lists[3][0][:2]) + [TR.pose_of(w, kw["tau"], "R3e38")]:
            n, d2 = _pin(O, Rt, src, tgt, rows)
            checked += n
            kinds |= {"zero" if x == 0 else "sub" if abs(x) < 2.0 ** -126 else "nan" if np.isnan(x) else "inf" if np.isinf(x) else "normal" for x in d2}
        print(name, sorted(kinds))
        if name == "a:300:-70":                                      # (normal: R3e38's products, 3e38 x 2^-70)
            assert {"zero", "sub"} <= kinds <= {"zero", "sub", "normal"}
        if name == "e":
            assert {"inf", "normal"} <= kinds                        # (an fma's product is exact: inf - inf does not arise in the chain)
    assert checked >= 1000


# ================================================================================================================================
# batches: sc_pose_info_batch (plain, slot, pairs), sc_assign_poses on a batch
# ================================================================================================================================
def batch_k(name):
    fam, *arg = name.partition("@")[0].split(":")
    return int(arg[1]) if fam == "a" else 0


def scaled_t(rt, k):
    out = np.array(rt, np.float32)
    out[9:] = scaled(out[9:], k)
    return out


def launches(cases, name_of=lambda c: c, size=40):
    """cases packed by launch (one sc_params: test_batch_tail_range_ref.tail_kw of the case's name), at most `size` a launch
    -> {id: (kw, [case, ...])} in first-seen order"""
    by = {}
    for case in cases:
        kw = TR.tail_kw(name_of(case))
        by.setdefault(tuple(sorted(kw.items())), (kw, []))[1].append(case)
    out = {}
    for kw, part in by.values():
        for lo in range(0, len(part), size):
            chunk = part[lo: lo + size]
            first = chunk[0] if isinstance(chunk[0], str) else "/".join(str(x) for x in chunk[0])
            out[first + (f"+{len(chunk) - 1}" if len(chunk) > 1 else "")] = (kw, chunk)
    return out


# -- pose-info: (name, pose) -> the input record is test_batch_tail_range_ref.polish_case's
INFO_CASES = ([(name, "winner") for name in R.NAMES] + sorted({(name, pose) for name, pose, _ in TR.POSES if (name, pose) not in (TR.ZEROS[:2], TR.E_MIRROR[:2])})
              + [TR.ZEROS[:2], TR.E_MIRROR[:2]])
INFO_LAUNCHES = launches(INFO_CASES, name_of=lambda c: c[0])


def info_case(pkg, O, name, pose):
    """-> (src, tgt, kw, input record, expected record of pose_info_ref.one)"""
    key = ("info batch", name, pose)
    if key not in _REF:
        src, tgt, kw, rin, _ = TR.polish_case(pkg, O, name, pose, TR.MAX_ITER)
        with np.errstate(**_QUIET):
            _REF[key] = (src, tgt, kw, rin, PI.one(O, src, tgt, rin["status"], rin["Rt"], kw["tau"]))
    return _REF[key]


def info_one_launch(pkg, O):
    """all magnitudes under the unit parameters in one launch -> (problems, input records, expected records)"""
    if "info one launch" not in _REF:
        problems = R.one_launch_problems(pkg)
        recs, _ = R.one_launch_ref(pkg, O)
        with np.errstate(**_QUIET):
            _REF["info one launch"] = (problems, recs, PI.batch(O, problems, recs, UNIT["tau"]))
    return _REF["info one launch"]


def test_the_pose_info_batch_cases_are_what_they_are_used_for(pkg, O):
    assert all(len(cases) <= 40 for _, cases in INFO_LAUNCHES.values()) and sum(len(c) for _, c in INFO_LAUNCHES.values()) == len(INFO_CASES)
    for n in R.SCENES:                                               # in window: inliers and a non-zero sse; the scaled blocks differ from k = 0's
        r0 = info_case(pkg, O, f"a:{n}:0", "winner")[4]
        for k in (-56, -30, 30, 62):
            src, tgt, kw, rin, r = info_case(pkg, O, f"a:{n}:{k}", "winner")
            assert len(src) == n <= 512 and int(r["status"]) == SC_OK and int(r["inliers"]) > 0 and float(r["sse"]) > 0, (n, k)
            assert not np.array_equal(r["info"].reshape(6, 6)[:3, :3], r0["info"].reshape(6, 6)[:3, :3]) and float(r["sse"]) != float(r0["sse"]), (n, k)
    z = info_case(pkg, O, *TR.ZEROS[:2])[4]
    print("ZEROS", int(z["inliers"]), float(z["sse"]), z["info"].reshape(6, 6).diagonal().tolist())
    assert int(z["status"]) == SC_OK and int(z["inliers"]) == 6 and float(z["sse"]) == 0.0 and z.tobytes() != bytes(320)
    assert z["info"].reshape(6, 6)[3:, 3:].tolist() == (6 * np.eye(3)).tolist() and not z["info"].reshape(6, 6)[:3].any()
    e = info_case(pkg, O, *TR.E_MIRROR[:2])[4]
    print("E_MIRROR", int(e["inliers"]), float(e["sse"]), float(np.abs(e["info"]).max()))
    assert int(e["status"]) == SC_OK and np.isfinite(e["info"]).all() and float(np.abs(e["info"]).max()) > 1e70
    # a:*:-70, the hostile poses and the statuses are there, and give what the contract says
    assert int(info_case(pkg, O, "a:300:-70", "winner")[4]["inliers"]) > 0
    assert info_case(pkg, O, "a:300:70", "winner")[4].tobytes() == _zero_info(SC_ENOHYP)
    for h, st in (("nan", SC_EINVAL), ("inf", SC_EINVAL), ("status:-1", SC_EINVAL), ("status:-5", SC_ENOHYP)):
        assert info_case(pkg, O, "a:300:64", h)[4].tobytes() == _zero_info(st), h
    for h in ("t3e38", "R3e38", "zero"):
        assert info_case(pkg, O, "a:300:64", h)[4].tobytes() == bytes(320), h
    problems, recs, exp = info_one_launch(pkg, O)
    assert len(problems) <= 40 and max(len(s) for s, _ in problems) <= 512
    assert (exp["inliers"] > 0).sum() >= 8 and (exp["status"] == SC_ENOHYP).sum() >= 10


def _zero_info(status):
    z = np.zeros((), PI.RESULT_DTYPE); z["status"] = status
    return z.tobytes()


# -- assign on a batch
ASSIGN_BATCH_NAMES = list(R.NAMES) + ["e@tau25"]
ASSIGN_LAUNCHES = launches(ASSIGN_BATCH_NAMES)
ASSIGN_KS = (1, 3, 16, 64)
# positions inside assign_ref.many's lists (none is 1, 5 or a far pose at 3 + 7 i)
BATCH_HOSTILE = {2: "R3e38", 4: "nan", 6: "zero", 9: "t3e38", 12: "inf", 13: "hostile"}
BATCH_STATUS = {8: SC_ENOHYP, 11: SC_EINVAL}


def assign_batch_poses(pkg, O, name, score_mode=0):
    """-> {K: (Rt (K, 12), statuses (K,))} for K in ASSIGN_KS, around the problem's reference winner (the identity where it has none)"""
    key = ("assign batch poses", name, score_mode)
    if key not in _REF:
        src, tgt, kw, rin, _ = TR.polish_case(pkg, O, name, "winner", TR.MAX_ITER, score_mode)
        _REF[key] = pose_lists(rin["Rt"], batch_k(name), kw["tau"], ASSIGN_SEED, ASSIGN_KS, BATCH_HOSTILE, BATCH_STATUS)
    return _REF[key]


def assign_batch_one(pkg, O, name, K, mode, score_mode=0):
    """-> (src, tgt, kw, Rt (K, 12), statuses (K,), (label, d2, records) of assign_ref.assign)"""
    key = ("assign batch", name, K, mode, score_mode)
    if key not in _REF:
        src, tgt, kw, _, _ = TR.polish_case(pkg, O, name, "winner", TR.MAX_ITER, score_mode)
        rt, st = assign_batch_poses(pkg, O, name, score_mode)[K]
        with np.errstate(all="ignore"):
            _REF[key] = (src, tgt, kw, rt, st, AR.assign(O, src, tgt, rt, kw["tau"], mode, None, st, score_mode))
    return _REF[key]


def batch_in_window(name):
    return name.startswith("a:") and in_window(batch_k(name), WIN_C2)


def test_assign_on_the_batch_discriminates_underflows_and_opens(pkg, O):
    assert all(len(names) <= 40 for _, names in ASSIGN_LAUNCHES.values())
    for name in ASSIGN_BATCH_NAMES:
        if not batch_in_window(name):
            continue
        n = int(name.split(":")[1])
        own = int(R.case_ref(pkg, O, name)[3]["best_count"])
        for K, dup in ((3, 2), (16, 5), (64, 5)):
            (lb, _, rb), (lf, _, rf) = (assign_batch_one(pkg, O, name, K, m)[5] for m in (AR.BEST, AR.FIRST))
            print(name, K, "labelled", _labelled(lb), "winner's count", own, "BEST != FIRST on", int((lb != lf).sum()))
            assert (lb != lf).any() and int(rb["count"][dup]) == 0 == int(rf["count"][dup]), (name, K)
            assert _labelled(lb) >= (100 if n == 512 else own // 2), (name, K)     # (the module docstring: why 512 and not 300)
            if K > 3:
                assert not rb["count"][sorted(BATCH_HOSTILE) + sorted(BATCH_STATUS)].any(), (name, K)
                assert rb["status"][sorted(BATCH_STATUS)].tolist() == [SC_ENOHYP, SC_EINVAL] and rb["status"][[4, 12]].tolist() == [SC_EINVAL] * 2
    # k = -70: tau^2 is the smallest subnormal, a residual below it is 0: every pose that claims a row ties, the lowest index wins
    for n in R.SCENES:
        name = f"a:{n}:-70"
        for K in (3, 16, 64):
            src, tgt, kw, rt, st, (lb, db, rb) = assign_batch_one(pkg, O, name, K, AR.BEST)
            lf = assign_batch_one(pkg, O, name, K, AR.FIRST)[5][0]
            valid = np.flatnonzero((st == SC_OK) & np.isfinite(rt).all(axis=1))
            with np.errstate(all="ignore"):
                D = AR.resid2(rt[valid], src, tgt)
                tau2 = AR.tau2_of(kw["tau"])
            rows = np.flatnonzero(lb >= 0)
            print(name, K, "labelled", len(rows), "tau2", float(tau2))
            assert len(rows) > 0 and 0 < tau2 < 2.0 ** -126
            # every pose near the winner — all but assign_ref.many's far ones (|t| + 1000 x 2^-70 squares to a normal number) and
            # the hostile ones — has a residual of 0 or a subnormal on every labelled row
            near = np.array([v % 7 != 3 and v not in BATCH_HOSTILE for v in valid]) | (K == 3)
            assert near.sum() >= min(K, 3) and (np.abs(D[near][:, rows]) < 2.0 ** -126).all()
            assert np.array_equal(lb, lf)
            assert np.array_equal(lb[rows], valid[np.argmax(D[:, rows] < tau2, axis=0)])     # the lowest valid index below tau^2
            assert (db[rows] == 0).all()
    # tau = 1e25: tau^2 = +inf; every row with a finite residual is labelled, a row whose every residual is inf or NaN is not
    for name in ("f:tau25", "e@tau25"):
        for K in (3, 64):
            src, tgt, kw, rt, st, (lb, db, rb) = assign_batch_one(pkg, O, name, K, AR.BEST)
            with np.errstate(all="ignore"):
                assert np.isinf(AR.tau2_of(kw["tau"]))
                D = AR.resid2(rt[(st == SC_OK) & np.isfinite(rt).all(axis=1)], src, tgt)
            fin = np.isfinite(D).any(axis=0)
            assert np.array_equal(lb >= 0, fin), (name, K)
            assert fin.all() == (name == "f:tau25"), (name, K)
    assert _labelled(assign_batch_one(pkg, O, "e@tau25", 64, AR.BEST)[5][0]) >= 290
    for mode in (1, 2):
        for name in TR.MODE_NAMES:
            rec = assign_batch_one(pkg, O, name, 16, AR.BEST, mode)[5][2]
            print("score mode", mode, name, rec["count"][:8].tolist(), rec["score"][:8].tolist())
        rec = assign_batch_one(pkg, O, "a:300:62", 16, AR.BEST, mode)[5][2]
        assert (rec["score"][rec["count"] > 0] != rec["count"][rec["count"] > 0]).any()
        rec = assign_batch_one(pkg, O, "f:tau25", 16, AR.BEST, mode)[5][2]
        assert int(rec["score"].sum()) == 100 * 1024                 # 1 / tau^2 = 0: every labelled row a perfect inlier


# ================================================================================================================================
# the guided matchers
# ================================================================================================================================
NS, NT, DIM = 130, 129, 33
G_KS = (-70, -64, -56, -30, 30, 62, 64, 70)
GATE_SUB = float(np.float32(2.0 ** -149))
GATE_MAX = float(np.finfo(np.float32).max)
GATE_FAR = 0.5                                  # the gate of the translated case: its coordinates are quantised to 2^-1, its residuals are
                                                # 0, 0.0625, 0.25, ...: 0.25 is gate^2 itself, and not admissible
E_ROWS = dict(src={10: (3e38, 0, 0), 70: (-3e38, 3e38, 0.1)}, tgt={11: (0, 3e38, 0), 70: (3e38, -3e38, 0.3), 90: (-3e38, -3e38, -3e38)})
B_KS = (-56, 62)                                # the boundary construction's scales
POSES_KS = (2, 5, 64)


def _f32(x):
    return float(np.float32(x))


def guided_case(name, seed=0):
    """name -> (match_guided_ref.Scene, gate): MG.scene at (130, 129), D = 33 (seed 0: MG.shared_scene's), its points, its pose's
    translation and its gate changed as the name says; the descriptors stay at unit scale"""
    key = ("guided", name, seed)
    if key in _REF:
        return _REF[key]
    base = MG.shared_scene(NS, NT, DIM) if seed == 0 else MG.scene(5100 + seed, NS, NT, DIM)
    sp, tp, rt, gate = base.src_pts.copy(), base.tgt_pts.copy(), np.array(base.Rt, np.float32), _f32(MG.GATE)
    fam, *arg = name.split(":")
    if fam == "scaled":
        k = int(arg[0])
        sp, tp, rt, gate = scaled(sp, k), scaled(tp, k), scaled_t(rt, k), float(np.float32(MG.GATE) * pow2(k))
    elif fam == "translated":
        es, et = int(arg[0]), int(arg[1])
        R64 = rt[:9].astype(np.float64).reshape(3, 3)
        rt[9:] = (rt[9:].astype(np.float64) + 2.0 ** et - R64 @ np.full(3, 2.0 ** es)).astype(np.float32)
        (sp, tp), gate = translated(sp, tp, es, et), GATE_FAR
    elif fam == "e":
        for i, v in E_ROWS["src"].items():
            sp[i] = v
        for j, v in E_ROWS["tgt"].items():
            tp[j] = v
        gate = GATE_MAX if arg == ["max"] else gate
    elif fam == "gate":
        gate = {"sub": GATE_SUB, "max": GATE_MAX}[arg[0]]
    elif fam != "unit":
        raise KeyError(name)
    _REF[key] = (MG.Scene(sp, base.fsrc, tp, base.ftgt, rt), gate)
    return _REF[key]


GUIDED_CASES = ["unit"] + [f"scaled:{k}" for k in G_KS] + ["translated:20:22", "e", "e:max", "gate:sub", "gate:max"]
GUIDED_IN_WINDOW = ["unit"] + [f"scaled:{k}" for k in G_KS if in_window(k, WIN_C2)]


def guided_problem(name, seed=0):
    key = ("guided problem", name, seed)
    if key not in _REF:
        sc, gate = guided_case(name, seed)
        with np.errstate(all="ignore"):
            _REF[key] = MG.Problem(*sc.args(), gate)
    return _REF[key]


def boundary_case(k):
    """test_gpu_match_guided.py::test_the_boundary_of_the_gate times 2^k: one source point at the origin, targets at gate, just
    inside it and just outside it, the identity pose; the nearer descriptors sit at the inadmissible targets -> (Scene, gate)"""
    half = np.float32(0.5)
    xs = np.array([half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1))], np.float32)
    tp = np.zeros((3, 3), np.float32); tp[:, 0] = scaled(xs, k)
    sc = MG.Scene(np.zeros((1, 3), np.float32), np.zeros((1, 1), np.float32), tp, np.array([[0.0], [1.0], [0.5]], np.float32),
                  AR.rt_of(np.eye(3), np.zeros(3)))
    return sc, float(half * pow2(k))


def poses_case(name, K, k=0):
    """the pose lists of sc_match_guided_poses on the unit scene times 2^k -> (Scene, poses (K, 12), statuses or None, gate):
    hostile   record 0 hostile (assign_ref.hostile), record 1 the scene's pose, the rest far shifts that admit nothing
    under     record 0 a close neighbour of the scene's pose, record 1 the scene's pose: at k = -70 both residuals underflow to 0 on
              the planted pairs and the label is 0, at k = 0 (run for comparison) record 1 is the nearer there
    off       record 0 the scene's pose under SC_ENOHYP (switched off), record 1 a neighbour of it, SC_GUIDE_POSE_STATUS set
    allhost   every record hostile"""
    sc, gate = guided_case("unit" if k == 0 else f"scaled:{k}")
    far = [scaled_t(AR.far(scaled_t(sc.Rt, -k)) + np.float32(i), k) for i in range(K)]
    poses, status = np.stack(far), None
    if name == "hostile":
        poses[0], poses[1] = AR.hostile(), sc.Rt
    elif name == "under":
        poses[0], poses[1] = scaled_t(AR.perturbed(scaled_t(sc.Rt, -k), 1, 32, angle=0.002, shift=0.001)[0], k), sc.Rt
    elif name == "off":
        near = scaled_t(AR.perturbed(scaled_t(sc.Rt, -k), 1, 31, angle=0.02, shift=0.01)[0], k)
        poses[0], poses[1] = sc.Rt, near
        status = np.zeros(K, np.int32); status[0] = SC_ENOHYP
    elif name == "allhost":
        poses[:] = AR.hostile()
    else:
        raise KeyError(name)
    return sc, np.ascontiguousarray(poses, np.float32), status, gate


POSES_CASES = [("hostile", 0), ("hostile", 62), ("under", -70), ("off", 0), ("off", -56), ("allhost", 0)]


def poses_problem(name, K, k):
    key = ("poses problem", name, K, k)
    if key not in _REF:
        sc, poses, status, gate = poses_case(name, K, k)
        with np.errstate(all="ignore"):
            _REF[key] = MP.Problem(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, poses, gate, None if status is None else status == SC_OK)
    return _REF[key]


def guided_batch(name):
    """four problems of the shape under one gate: seeds 0 .. 3 of the case -> (match_guided_batch_ref.Batch, gate)"""
    key = ("guided batch", name)
    if key not in _REF:
        cases = [guided_case(name, seed) for seed in range(4)]
        _REF[key] = (GB.Batch([c[0] for c in cases]), cases[0][1])
    return _REF[key]


PAIR_SIZES = (65, 130, 100, 129)
PAIR_LIST = np.array([(0, 1), (2, 3), (1, 0), (3, 3), (0, 1)], np.uint32)


def guided_table(name):
    """sets of 65 to 130 rows in one frame, changed as guided_case changes a scene -> (pairs_ref-style table with poses, gate)"""
    key = ("guided table", name)
    if key not in _REF:
        fam, *arg = name.split(":")
        k = int(arg[0]) if fam == "scaled" else 0
        sets = []
        for n in PAIR_SIZES:
            rng = np.random.default_rng(8900 + n)
            sets.append((rng.random((n, 3)).astype(np.float32), rng.normal(size=(n, DIM)).astype(np.float32)))
        ident = AR.rt_of(np.eye(3), np.zeros(3))
        poses = np.ascontiguousarray(AR.perturbed(ident, len(PAIR_LIST), 43, angle=0.05, shift=0.02), np.float32)
        gate = _f32(MG.GATE)
        if fam == "scaled":
            sets = [(scaled(p, k), f) for p, f in sets]
            poses[:, 9:] = scaled(poses[:, 9:], k)
            gate = float(np.float32(MG.GATE) * pow2(k))
        elif fam == "translated":                                    # one frame: every set moves by the same 2^es
            es = int(arg[0])
            sets = [((p + pow2(es)).astype(np.float32), f) for p, f in sets]
            for p in range(len(poses)):
                R64 = poses[p, :9].astype(np.float64).reshape(3, 3)
                poses[p, 9:] = (poses[p, 9:].astype(np.float64) + 2.0 ** es - R64 @ np.full(3, 2.0 ** es)).astype(np.float32)
            gate = GATE_FAR / 4
        elif fam == "e":
            for s, rows in ((0, E_ROWS["src"]), (1, E_ROWS["tgt"])):
                pts = sets[s][0].copy()
                for i, v in rows.items():
                    pts[i % len(pts)] = v
                sets[s] = (pts, sets[s][1])
            gate = GATE_MAX if arg == ["max"] else gate
        elif fam == "gate":
            gate = {"sub": GATE_SUB, "max": GATE_MAX}[arg[0]]
        elif fam != "unit":
            raise KeyError(name)
        set_off = np.concatenate([[0], np.cumsum([len(p) for p, _ in sets])]).astype(np.uint32)
        _REF[key] = (dict(sets=sets, pts=np.concatenate([p for p, _ in sets]), feat=np.concatenate([f for _, f in sets]), set_off=set_off,
                          poses=poses), gate)
    return _REF[key]


def _tiles(adm):
    """which (row block of 128, column tile of 64) of a (130, 129) mask hold an admissible cell"""
    return [[bool(adm[r0: r0 + 128, c0: c0 + 64].any()) for c0 in (0, 64, 128)] for r0 in (0, 128)]


def test_the_guided_cases_are_what_they_are_used_for():
    plain = {}
    for name in GUIDED_CASES:
        sc, gate = guided_case(name)
        prob = guided_problem(name)
        n1 = len(prob.match(knn=1)[0])
        tiles = _tiles(prob.adm)
        with np.errstate(all="ignore"):
            g2 = MG.gate2_of(gate)
        print(name, "gate2", float(g2), "admissible", int(prob.adm.sum()), "of", prob.adm.size, "knn=1 keeps", n1, "tiles", tiles,
              "g2: zeros", int((prob.g2 == 0).sum()), "inf", int(np.isinf(prob.g2).sum()), "nan", int(np.isnan(prob.g2).sum()))
        assert sc.src_pts.shape == (NS, 3) and sc.tgt_pts.shape == (NT, 3) and sc.fsrc.shape == (NS, DIM)
        assert all(np.isfinite(a).all() for a in sc.args())          # finite inputs: no case may raise the flag
        plain[name] = n1
        if name in GUIDED_IN_WINDOW or name in ("translated:20:22", "e"):
            assert 0 < n1 < NS, name                                 # the gate keeps something and drops something
            flat = [t for row in tiles for t in row]
            assert True in flat and False in flat, (name, tiles)     # a whole tile of a row block is skipped, another is computed
    for name in GUIDED_IN_WINDOW[1:]:                                # in window the mask is the unit scene's
        assert np.array_equal(guided_problem(name).adm, guided_problem("unit").adm), name
    # outside the window of C2: the residuals underflow (ties at 0, a gate of a few subnormal steps) or overflow
    lo, hi = guided_problem("scaled:-70"), guided_problem("scaled:70")
    # (the 43 planted pairs are 1e-2 apart: 1e-4 x 2^-140 is below half the smallest subnormal)
    assert (np.abs(lo.g2) < 2.0 ** -126).all() and (lo.g2 == 0).sum() >= 40 and not np.array_equal(lo.adm, guided_problem("unit").adm)
    assert np.isinf(hi.g2).sum() > 10000 and np.isinf(MG.gate2_of(guided_case("scaled:70")[1])) and np.array_equal(hi.adm, np.isfinite(hi.g2))
    # quantised coordinates: exact ties in g2 among the admissible cells
    far = guided_problem("translated:20:22")
    vals = far.g2[far.adm]
    assert len(np.unique(vals)) < len(vals) // 2
    # the rows at +-3e38: non-finite residuals, never admissible, whatever the gate
    for name in ("e", "e:max"):
        e = guided_problem(name)
        bad = ~np.isfinite(e.g2)
        assert bad[10].all() and bad[70].all() and bad[:, 11].all() and bad[:, 90].all() and not e.adm[bad].any() and bad.sum() < e.adm.size // 10
    assert np.array_equal(guided_problem("e:max").adm, np.isfinite(guided_problem("e:max").g2))
    # the two extreme gates
    sub, top = guided_problem("gate:sub"), guided_problem("gate:max")
    assert MG.gate2_of(GATE_SUB) == 0 and not sub.adm.any() and all(len(sub.match(**kw)[0]) == 0 for kw in MG.MODES)
    assert np.isinf(MG.gate2_of(GATE_MAX)) and top.adm.all()
    sc = guided_case("gate:max")[0]
    for kw in MG.MODES:
        c, d, _ = top.match(**kw)
        pc, pd = match_ref.match(sc.fsrc, sc.ftgt, **kw)[:2]
        assert np.array_equal(c, pc) and d.tobytes() == np.asarray(pd, np.float32).tobytes(), kw


@pytest.mark.parametrize("k", B_KS)
def test_the_scaled_boundary_flips_exactly_the_planted_pair(k):
    sc, gate = boundary_case(k)
    with np.errstate(all="ignore"):
        prob = MG.Problem(*sc.args(), gate)
        g2 = MG.gate2_of(gate)
    assert 2.0 ** -126 < g2 < np.inf and prob.g2[0, 0] == g2 and prob.g2[0, 1] < g2 < prob.g2[0, 2]
    assert prob.g2[0, 1] == np.nextafter(g2, np.float32(0)) or prob.g2[0, 1] < g2      # one step of the coordinate: at most two of its square
    assert prob.adm.tolist() == [[False, True, False]]
    assert prob.match(knn=4)[0].tolist() == [[0, 1]]


def test_the_pose_lists_of_the_poses_matcher_are_what_they_are_used_for():
    for name, k in POSES_CASES:
        for K in POSES_KS:
            sc, poses, status, gate = poses_case(name, K, k)
            prob = poses_problem(name, K, k)
            c, d, g, lab = prob.match(knn=1)
            print(name, k, K, "kept", len(c), "labels", np.unique(lab).tolist())
            assert np.isfinite(poses).all() and len(poses) == K
            if name == "hostile":                                    # record 0 admits nothing, yields inf / NaN; record 1 labels everything kept
                assert not prob.adm_k[0].any() and len(c) > 0 and (lab == 1).all() and np.isfinite(g).all()
                single = guided_problem("unit" if k == 0 else f"scaled:{k}").match(knn=1)
                assert np.array_equal(c, single[0]) and g.tobytes() == single[2].tobytes()
            elif name == "under":                                    # where both residuals underflow to 0 the label is the lower index,
                unit = poses_problem("under", K, 0).match(knn=1)     # though at unit scale record 1 (the scene's pose) is the nearer
                both = {(int(i), int(j)) for (i, j), x, la in zip(c, g, lab) if x == 0 and la == 0}
                assert len(both) >= 10 and (np.abs(g) < 2.0 ** -126).all()
                assert sum((int(i), int(j)) in both and la == 1 for (i, j), la in zip(unit[0], unit[3])) >= 5
            elif name == "off":                                      # the switched-off record would have admitted more, and is not looked at
                assert len(c) > 0 and (lab == 1).all() and not prob.adm_k[0].any()
                full = guided_problem("unit" if k == 0 else f"scaled:{k}")
                assert full.adm.sum() > 0 and not np.array_equal(full.adm, prob.adm)
            else:
                assert len(c) == 0 and not prob.adm.any()


def test_the_guided_batch_and_table_are_what_they_are_used_for():
    for name in ("unit", "scaled:-56", "scaled:62", "scaled:-70", "scaled:70", "translated:20:22", "e", "gate:sub", "gate:max"):
        batch, gate = guided_batch(name)
        with np.errstate(all="ignore"):
            exp = GB.match_batch(batch, gate, knn=1)
        tab, tgate = guided_table(name)
        with np.errstate(all="ignore"):
            pexp = GB.match_batch(GB.expand(tab, PAIR_LIST, tab["poses"]), tgate, knn=1)
        print(name, "batch", exp[3].tolist(), "pairs", pexp[3].tolist())
        assert len(batch) == 4 and not exp[3][:, 1].any() and not pexp[3][:, 1].any()
        assert all(65 <= len(p) <= 130 for p, _ in tab["sets"])
        if name in ("unit", "scaled:-56", "scaled:62", "translated:20:22", "e"):
            assert all(0 < n < NS for n in exp[3][:, 0]) and (pexp[3][:, 0] > 0).all(), name
        if name == "gate:sub":
            assert not exp[3].any() and not pexp[3].any()
        if name == "gate:max":
            assert (exp[3][:, 0] == NS).all()
    a, b = (GB.match_batch(guided_batch(n)[0], guided_batch(n)[1], knn=1) for n in ("unit", "scaled:62"))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])


def test_no_problem_is_over_large(pkg, O):
    """n <= 512 per batch problem, frames of 300 (500: the sparse scene) and 1500, matchers at 130 x 129."""
    assert max(len(TR.polish_case(pkg, O, name)[0]) for name in ASSIGN_BATCH_NAMES) <= 512
    assert max(len(info_case(pkg, O, *c)[0]) for c in INFO_CASES[:len(R.NAMES)]) <= 512
    assert (NS, NT) == (130, 129) and batch_ref.TRI_CAP >= max(int(R.case_ref(pkg, O, n)[3]["tri_total"]) for n in R.NAMES)
