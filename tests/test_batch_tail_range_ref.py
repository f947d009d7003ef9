"""CPU suite: the inputs of tests/test_gpu_polish_batch_range.py and tests/test_gpu_instances_batch_range.py — sc_polish_batch (plain,
slot and pairs forms) and sc_register_instances_batch (plain and features forms) at the ends of the fp32 range — and what the
REFERENCE alone says about them.

The two GPU files compare the kernels with tests/polish_batch_ref.py and tests/instances_batch_ref.py bit for bit; that is only worth
something if the inputs leave the beaten path: every way a polish can stop, every status, a pose that is caller data and hostile,
rounds that lose the second motion, fill every plane, take a winner with a claimed vertex, stop on min_score — and if no problem
is so large that one workgroup runs long.  All of these are conditions on the reference, asserted here.

The scenes, families and parameter sets of the polish are those of tests/test_batch_range_ref.py (imported, not copied); the input
pose of a case is the reference's batch record unless the POSES table gives another one:
  shift:c   the winner's pose with t + c * tau * (1, -1, 0.5) / 1.5 (fp32): |shift| = c tau, so c < 1 keeps most inliers, c = 1.5 few
            and c = 3 none;
  t3e38     the winner's R with t = (3e38, 3e38, 3e38): R p + t is inf or 3e38, never an inlier;
  R3e38     every entry of R 3e38, t = 0: R p overflows to +-inf row by row, inf - inf = NaN in the residual;
  zero      R = 0, t = 0: finite, and far from every point of a unit scene;
  nan, inf  one non-finite entry in the winner's Rt under status SC_OK: SC_EINVAL from the pose alone;
  status:s  the winner's pose under status s (SC_EINVAL, SC_ENOHYP): passed through, whatever the pose is worth.

The "not finite: declined" exit of the refit's solve IS reachable from finite inputs on the reference (ZEROS below): the six exact
zeros of family b under the zero pose and tau = 2^-60 are the pose's only inliers, p - pc = q - qc = 0, H = 0, and the two dominant
columns have length 0: 0 / 0.  Rows at +-3e38 cannot reach it: the sums are fp64, (3e38)^2 = 9e76 is far from its end, so a pose that
makes such a row an inlier (E_MIRROR: R = -I, t = (0, 0, 0.4) maps src[70] onto tgt[70] exactly; tau = 1e25 makes every finite row one)
gets a finite refit — that case is kept because its centroids and H are of order 1e36 and 1e74.

The instances scenes are instances_batch_ref.scene (two motions) at n = 128, 257, 512, T = 200, max_instances 4, min_score 4 (4 x 256
in the truncated score modes: 1024 per perfect inlier there).
"""
import numpy as np

import batch_ref
import instances_batch_ref as IR
import polish_batch_ref as PB
import test_batch_range_ref as R
from test_range_oracle import UNIT, WIN_REGISTER, in_window, pow2, same_bits_nan, scaled, scaled_kw, translated

SC_OK, SC_EINVAL, SC_ENOHYP = batch_ref.SC_OK, batch_ref.SC_EINVAL, batch_ref.SC_ENOHYP
T = R.T
MAX_ITER = 16
_REF = {}
_QUIET = dict(over="ignore", under="ignore", divide="ignore", invalid="ignore")


# ---- sc_polish_batch: the cases ----------------------------------------------------------------------------------------------------
SHIFT_NAMES = ("a:300:0", "a:300:-56", "a:300:62", "a:300:-64", "a:300:64", "a:512:-70", "e", "c:20:22", "b:far62")
HOSTILE_NAMES = ("a:300:0", "a:300:-64", "a:300:64", "e")
SHIFTS = [(c, mi) for c in ("0.5", "0.9", "1.5") for mi in (1, 2, MAX_ITER)] + [("3.0", MAX_ITER)]
HOSTILE = ("t3e38", "R3e38", "zero", "nan", "inf", "status:-1", "status:-5")
ZEROS = ("b:minlen0@tau-60", "zero", MAX_ITER)     # the solve's own "not finite" exit, from finite inputs
E_MIRROR = ("e@tau25", "mirror", MAX_ITER)         # a +-3e38 row among the inliers: a finite refit
POSES = ([(name, "shift:" + c, mi) for name in SHIFT_NAMES for c, mi in SHIFTS] +
         [(name, h, MAX_ITER) for name in HOSTILE_NAMES for h in HOSTILE] + [ZEROS, E_MIRROR])
MODE_NAMES = ("f:tau-30", "f:tau25", "a:300:-56", "a:300:62")   # tests/test_gpu_batch_range.py::test_score_modes' cases
MODE_POSES = ("winner", "shift:0.9", "t3e38", "R3e38", "zero")


def tail_kw(name):
    """the parameters of a polish case's launch: test_batch_range_ref.case_kw, `@tau...` replaces tau"""
    base, _, over = name.partition("@")
    kw = R.case_kw(base)
    if over:
        kw["tau"] = {"tau-60": float(pow2(-60)), "tau25": R.F_CASES["tau25"]["tau"]}[over]
    return kw


def pose_of(rt0, tau, pose):
    """the input pose of a table row: rt0 is the reference's winner (12 floats), tau the launch's"""
    rt = np.ascontiguousarray(rt0, np.float32).copy()
    big = np.float32(3e38)
    if pose.startswith("shift:"):
        with np.errstate(**_QUIET):
            rt[9:] = rt[9:] + np.float32(float(pose[6:])) * np.float32(tau) * np.array([1, -1, .5], np.float32) / np.float32(1.5)
    elif pose == "t3e38":
        rt[9:] = big
    elif pose == "R3e38":
        rt[:9], rt[9:] = big, 0
    elif pose == "zero":
        rt[:] = 0
    elif pose == "mirror":
        rt[:] = (-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0.4)
    elif pose == "nan":
        rt[5] = np.nan
    elif pose == "inf":
        rt[10] = -np.inf
    elif pose != "winner":
        raise KeyError(pose)
    return rt


def polish_case(pkg, O, name, pose="winner", max_iter=MAX_ITER, mode=0):
    """-> (src, tgt, kw, input record, (record, mask) of polish_batch_ref.one), once per session; never modified.  A pose other than
    the winner's is handed in under status SC_OK, whatever the registration said."""
    key = ("polish", name, pose, max_iter, mode)
    if key not in _REF:
        base = name.partition("@")[0]
        src, tgt, _, rec, _ = R.case_ref(pkg, O, base, mode)
        kw = tail_kw(name)
        rin = rec.copy()
        if pose.startswith("status:"):
            rin["status"] = int(pose[7:])
        elif pose != "winner":
            rin["status"], rin["Rt"] = SC_OK, pose_of(rec["Rt"], kw["tau"], pose)
        with np.errstate(**_QUIET):
            _REF[key] = (src, tgt, kw, rin, PB.one(O, src, tgt, rin, kw["tau"], mode, max_iter))
    return _REF[key]


def polish_groups(cases):
    """cases: (name, pose, max_iter) -> the cases packed by launch (one sc_params, one max_iter): [(kw, max_iter, [case, ...]), ...]"""
    out = {}
    for case in cases:
        kw = tail_kw(case[0])
        out.setdefault((tuple(sorted(kw.items())), case[2]), (kw, case[2], []))[2].append(case)
    return list(out.values())


def _prow(rec):
    return tuple(int(rec[f]) for f in PB.FIELDS)


def _how(rec):
    """(status, stop, refitted at all) of a polish record"""
    return int(rec["status"]), int(rec["stop"]), int(rec["iters"]) > 0


FIXED, DECLINED, MAXED = PB.STOP_FIXED, PB.STOP_DECLINED, PB.STOP_MAX_ITER
# (score0, score, iters, stop) of the winner's polish — whoever changes a scene or a parameter sees here what the GPU file no longer covers
PIN = {"a:300:0": (85, 87, 3, FIXED), "a:300:-64": (88, 87, None, None), "a:512:-70": (77, 82, 5, None), "a:192:66": (37, 55, None, None),
       "c:20:22": (22, 2, 9, DECLINED), "e": (84, 86, None, None)}


def test_the_winners_polish_stops_in_every_way(pkg, O):
    """Every name of test_batch_range_ref.NAMES at max_iter 16 from the winner's pose."""
    hows, passed = set(), set()
    for name in R.NAMES:
        src, tgt, kw, rin, (rec, mask) = polish_case(pkg, O, name)
        print(name, "in", int(rin["status"]), int(rin["best_count"]), "| polish", _prow(rec), int(mask.sum()))
        hows.add(_how(rec))
        if rin["status"] != SC_OK:
            passed.add(name)
            assert _prow(rec) == (int(rin["status"]), 0, 0, 0, DECLINED) and rec["Rt"].tobytes() == batch_ref.IDENT.tobytes() and not mask.any()
        else:
            assert rec["status"] == SC_OK and int(rec["score0"]) == int(rin["best_count"]), name   # score0 IS the batch record's count
            assert int(mask.sum()) == int(rec["score"]), name                                      # ... and in mode 0 the score the mask's
    for name, (s0, s1, iters, stop) in PIN.items():
        rec = polish_case(pkg, O, name)[4][0]
        assert (int(rec["score0"]), int(rec["score"])) == (s0, s1), (name, _prow(rec))
        assert iters is None or int(rec["iters"]) == iters, (name, _prow(rec))
        assert stop is None or int(rec["stop"]) == stop, (name, _prow(rec))
    assert {f"a:{n}:70" for n in R.SCENES} | {"c:22:24", "c:24:20", "f:tau-30", "f:tcmp1", "f:sigma-30", "f:minlen38"} <= passed
    assert {(SC_OK, FIXED, True), (SC_OK, DECLINED, True), (SC_ENOHYP, DECLINED, False)} <= hows, hows


def test_the_pose_table_reaches_every_stop_at_every_scale(pkg, O):
    """The shifted and the hostile poses: per name which (stop, refitted) combinations the table reaches, and the rows pinned."""
    per = {}
    for name, pose, mi in POSES:
        rec, mask = polish_case(pkg, O, name, pose, mi)[4]
        print(name, pose, mi, _prow(rec), int(mask.sum()))
        per.setdefault(name, set()).add(_how(rec) + (mi,))
        if pose.startswith("shift:") and mi < MAX_ITER and rec["stop"] == MAXED:
            assert int(rec["iters"]) == mi, (name, pose, mi)
    for name in SHIFT_NAMES:
        if name == "c:20:22":      # |t| = 2^22: the shift is below half an ulp of t, the pose is the winner's
            assert all(polish_case(pkg, O, name, "shift:" + c, mi)[3]["Rt"].tobytes() == polish_case(pkg, O, name)[3]["Rt"].tobytes() for c, mi in SHIFTS)
            continue
        hows = {h[:3] for h in per[name]}
        assert (SC_OK, MAXED, True) in hows and (SC_OK, DECLINED, False) in hows, (name, hows)
        assert any(h[:3] == (SC_OK, MAXED, True) and h[3] == 1 for h in per[name]) and any(h[:3] == (SC_OK, MAXED, True) and h[3] == 2 for h in per[name]), name
        rec = polish_case(pkg, O, name, "shift:3.0", MAX_ITER)[4][0]
        assert _prow(rec)[2:] == (int(rec["score0"]), 0, DECLINED) and int(rec["score0"]) < 3, (name, _prow(rec))   # declined before the first
    assert any((SC_OK, FIXED, True) == h[:3] for name in SHIFT_NAMES for h in per[name])
    rec = polish_case(pkg, O, "a:300:-64", "shift:1.5", MAX_ITER)[4][0]
    assert _prow(rec) == (SC_OK, 2, 2, 0, DECLINED)
    rec = polish_case(pkg, O, "a:512:-70", "shift:0.5", MAX_ITER)[4][0]
    assert (int(rec["iters"]), int(rec["stop"])) == (7, FIXED), _prow(rec)
    # the hostile poses
    for name in HOSTILE_NAMES:
        src = polish_case(pkg, O, name)[0]
        for h in ("t3e38", "R3e38", "zero"):
            _, _, _, rin, (rec, mask) = polish_case(pkg, O, name, h, MAX_ITER)
            assert np.isfinite(rin["Rt"]).all() and _prow(rec) == (SC_OK, 0, 0, 0, DECLINED) and not mask.any(), (name, h, _prow(rec))
            assert rec["Rt"].tobytes() == rin["Rt"].tobytes(), (name, h)                 # a declined refit keeps the input pose
        for h in ("nan", "inf"):
            _, _, _, rin, (rec, mask) = polish_case(pkg, O, name, h, MAX_ITER)
            assert rin["status"] == SC_OK and _prow(rec) == (SC_EINVAL, 0, 0, 0, DECLINED) and not mask.any(), (name, h)
            assert rec["Rt"].tobytes() == batch_ref.IDENT.tobytes()
        for st in (SC_EINVAL, SC_ENOHYP):
            _, _, _, rin, (rec, mask) = polish_case(pkg, O, name, f"status:{st}", MAX_ITER)
            assert np.isfinite(rin["Rt"]).all() and rin["best_count"] > 3 and _prow(rec) == (st, 0, 0, 0, DECLINED) and not mask.any(), (name, st)
            assert rec["Rt"].tobytes() == batch_ref.IDENT.tobytes()
    # R3e38 is hostile for the reason meant: at 2^64 every product R_rc p_c is +-inf and a row of them sums to inf or to NaN; on
    # the unit scene R p is finite (|x + y + z| < 1.13) and merely far away
    src, _, _, rin, _ = polish_case(pkg, O, "a:300:64", "R3e38", MAX_ITER)
    with np.errstate(**_QUIET):
        prod = rin["Rt"][:3][None, :] * src
        moved = (prod[:, 0] + prod[:, 1]) + prod[:, 2]
    assert np.isinf(prod).all() and np.isinf(moved).any() and np.isnan(moved).any()


def test_the_solves_not_finite_exit_is_reached_from_finite_inputs(pkg, O):
    """ZEROS: six inliers (score0 = 6 >= 3: not the count's exit), all of them (0, 0, 0) -> (0, 0, 0): H = 0, the refit returns
    `not done`, declined without a refit, pose, score and mask stay.  E_MIRROR: a row at +-3e38 among the 297 inliers, and the refit is
    finite (and so far off that the next one is declined by the count)."""
    src, tgt, kw, rin, (rec, mask) = polish_case(pkg, O, *ZEROS)
    print("zeros", _prow(rec), np.flatnonzero(mask).tolist())
    assert np.isfinite(src).all() and np.isfinite(tgt).all() and not rin["Rt"].any() and 0 < np.float32(kw["tau"]) ** 2
    assert _prow(rec) == (SC_OK, 6, 6, 0, DECLINED) and np.flatnonzero(mask).tolist() == list(range(R.B_ZERO.start, R.B_ZERO.stop))
    assert not src[R.B_ZERO].any() and not tgt[R.B_ZERO].any() and rec["Rt"].tobytes() == rin["Rt"].tobytes()
    done, _ = O.refine(src, tgt, mask, rin["Rt"])
    assert not done
    src, tgt, kw, rin, (rec, mask) = polish_case(pkg, O, *E_MIRROR)
    print("e mirror", _prow(rec), int(mask.sum()), rec["Rt"])
    with np.errstate(**_QUIET):
        before = O.mask(src, tgt, rin["Rt"], kw["tau"])
    assert before[70] == 1 and abs(float(src[70, 0])) > 1e38          # the row IS an inlier of the input pose
    assert _prow(rec) == (SC_OK, 297, 0, 1, DECLINED) and np.isfinite(rec["Rt"]).all() and not mask.any()  # one finite refit; it loses every inlier


def test_score_modes_of_the_polish(pkg, O):
    """1 / tau^2 and 1 / tau are inf (f:tau-30), 0 (f:tau25), 2^-120 / 2^60-ish (a:300:62 / -56) in the truncated modes."""
    for mode in (1, 2):
        for name in MODE_NAMES:
            for pose in MODE_POSES:
                _, _, kw, rin, (rec, mask) = polish_case(pkg, O, name, pose, MAX_ITER, mode)
                print(mode, name, pose, _prow(rec), int(mask.sum()))
                if pose == "winner" and rin["status"] == SC_OK:
                    assert int(rec["score0"]) == int(rin["best_count"]), (mode, name)
        assert polish_case(pkg, O, "f:tau-30", "winner", MAX_ITER, mode)[4][0]["status"] == SC_ENOHYP
        rec = polish_case(pkg, O, "f:tau25", "winner", MAX_ITER, mode)[4][0]
        assert rec["status"] == SC_OK and int(rec["score"]) == 100 * 1024             # 1 / tau^2 = 0: every point a perfect inlier
        a, b = (polish_case(pkg, O, n, "winner", MAX_ITER, mode)[4][0] for n in ("a:300:-56", "a:300:62"))
        assert _prow(a) == _prow(b) and int(a["score"]) > 1024                        # both inside the window: covariant


def test_the_polish_inside_the_window_is_covariant(pkg, O):
    """What the GPU file's metamorphic check rests on: winner and shifted poses at k are those at k = 0, t times 2^k."""
    for n in R.SCENES:
        for pose in ("winner", "shift:0.5", "shift:1.5"):
            r0, m0 = polish_case(pkg, O, f"a:{n}:0", pose)[4]
            for k in R.metamorphic_ks():
                r, m = polish_case(pkg, O, f"a:{n}:{k}", pose)[4]
                assert _prow(r) == _prow(r0) and np.array_equal(m, m0), (n, k, pose)
                assert same_bits_nan(r["Rt"][:9], r0["Rt"][:9]) and same_bits_nan(r["Rt"][9:], r0["Rt"][9:] * pow2(k)), (n, k, pose)


def polish_one_launch(pkg, O):
    """All magnitudes under the unit parameters in ONE launch: test_batch_range_ref.one_launch_problems and their records, polished.
    -> (problems, input records, (records, masks))"""
    if "polish one launch" not in _REF:
        problems = R.one_launch_problems(pkg)
        recs, _ = R.one_launch_ref(pkg, O)
        with np.errstate(**_QUIET):
            _REF["polish one launch"] = (problems, recs, PB.batch(O, problems, recs, UNIT["tau"], 0, MAX_ITER))
    return _REF["polish one launch"]


def test_the_polish_of_all_magnitudes_in_one_launch(pkg, O):
    problems, recs, (out, masks) = polish_one_launch(pkg, O)
    st = out["status"].tolist()
    print("one launch:", len(st), "problems,", [_prow(r) for r in out])
    assert len(problems) <= 40 and st == recs["status"].tolist() and st.count(SC_OK) >= 8 and st.count(SC_ENOHYP) >= 10
    assert len({_how(r) for r in out}) >= 3


# ---- sc_register_instances_batch: the cases --------------------------------------------------------------------------------------
I_SCENES = ((128, .5), (257, .4), (512, .3))
I_KS = (0, -70, -64, -56, -30, 30, 62, 64, 66)
I_NAMES = [f"s:{n}:{k}" for k in I_KS for n, _ in I_SCENES] + ["e:257", "c:257:20:22", "far:257:62", "far:512:62"]
I_MODE_NAMES = [f"s:{n}:{k}" for k in (-56, 62) for n, _ in I_SCENES]
MAX_INSTANCES = 4
FOUND = {0: (2, 2, 2), -56: (2, 2, 2), -30: (2, 2, 2), 30: (2, 2, 2), 62: (2, 2, 2), -64: (1, 1, 1), -70: (2, 2, 3), 64: (2, 2, 2), 66: (2, 4, 4)}


def min_score_of(mode):
    return 4 if mode == 0 else 4 * 256


def inst_kw(name):
    fam, *arg = name.split(":")
    return dict(scaled_kw(int(arg[1])) if fam == "s" else UNIT, max_triangles=T)     # (e, c, far: the unit parameters)


def inst_input(pkg, name):
    """name -> (src, tgt, kw).  s:n:k the scene times 2^k; e:257 rows at +-3e38 planted as in family e; c:257:es:et translated;
    far:n:k rows 64 .. 127 times 2^k inside the unit scene (family b's far62)."""
    fam, *arg = name.split(":")
    n = int(arg[0])
    src, tgt = (x.copy() for x in IR.scene(pkg, n, dict(I_SCENES)[n]))
    if fam == "s":
        src, tgt = scaled(src, int(arg[1])), scaled(tgt, int(arg[1]))
    elif fam == "e":
        big = np.float32(3e38)
        src[10] = (big, 0, 0); src[70] = (-big, big, 0.1)
        tgt[11] = (0, big, 0); tgt[70] = (big, -big, 0.3); tgt[90] = (-big, -big, -big)
    elif fam == "c":
        src, tgt = translated(src, tgt, int(arg[1]), int(arg[2]))
    elif fam == "far":
        src[64:128] = scaled(src[64:128], int(arg[1])); tgt[64:128] = scaled(tgt[64:128], int(arg[1]))
    else:
        raise KeyError(name)
    return src, tgt, inst_kw(name)


def inst_ref(pkg, O, name, mode=0):
    """(src, tgt, kw, planes, label, found, info) of one case on the reference, once per session; never modified."""
    key = ("inst", name, mode)
    if key not in _REF:
        src, tgt, kw = inst_input(pkg, name)
        info = {}
        with np.errstate(**_QUIET):
            planes, label, found = IR.one(O, src, tgt, kw, mode, MAX_INSTANCES, min_score_of(mode), info)
        _REF[key] = (src, tgt, kw, planes, label, found, info)
    return _REF[key]


def inst_groups(names=I_NAMES):
    out = {}
    for name in names:
        kw = inst_kw(name)
        out.setdefault(tuple(sorted(kw.items())), (kw, []))[1].append(name)
    return list(out.values())


def inst_metamorphic_ks():
    return [k for k in I_KS if k and in_window(k, WIN_REGISTER)]


def _irow(planes, found):
    return int(found), [int(x) for x in planes["best_count"]], [int(x) for x in planes["best_rank"]]


def test_the_instances_cases_are_what_they_are_used_for(pkg, O):
    ends, claimed, totals = {}, [], {}
    for mode, names in ((0, I_NAMES), (1, I_MODE_NAMES), (2, I_MODE_NAMES)):
        for name in names:
            src, tgt, kw, planes, label, found, info = inst_ref(pkg, O, name, mode)
            print(mode, name, _irow(planes, found), "tri", int(planes[0]["tri_total"]), "kept", int(planes[0]["tri_kept"]), info.get("end"),
                  "claimed vertex" if info.get("claimed_vertex") else "")
            assert int(planes[0]["tri_total"]) <= batch_ref.TRI_CAP, name
            assert [int((label == j).sum()) for j in range(found)] == [int(x) for x in planes[:found]["best_count"]] or mode
            ends[mode, name] = info.get("end")
            totals[mode, name] = int(planes[0]["tri_total"])
            if info.get("claimed_vertex"):
                claimed.append((mode, name))
    for k, want in FOUND.items():
        assert tuple(inst_ref(pkg, O, f"s:{n}:{k}")[5] for n, _ in I_SCENES) == want, k
    assert [totals[0, f"s:{n}:66"] for n, _ in I_SCENES] == [16, 16, 62]                       # lists shorter than T
    assert max(totals.values()) == 57738
    assert (0, "s:512:-70") in claimed, claimed                                              # a later winner has a claimed vertex
    assert ends[0, "s:257:66"] == ends[0, "s:512:66"] == ("max_instances", MAX_INSTANCES)  # every plane filled
    low = {key: e for key, e in ends.items() if e and e[0] == "min_score" and 0 < e[1]}
    assert (0, "s:128:-64") in low and all(e[1] < min_score_of(m) for (m, _), e in low.items()), ends   # ends on min_score, a score left
    # the second motion really is lost at -64, and the graph is another one at 64
    for n, _ in I_SCENES:
        p0, pm, pp = (inst_ref(pkg, O, f"s:{n}:{k}")[3] for k in (0, -64, 64))
        assert pm[1]["status"] == SC_ENOHYP and pm[1]["Rt"].tobytes() == batch_ref.IDENT.tobytes() and p0[1]["status"] == SC_OK
        assert int(pp[0]["edges"]) != int(p0[0]["edges"]) and [int(x) for x in pp[:2]["best_rank"]] != [int(x) for x in p0[:2]["best_rank"]]
    # e:257 and c:257 are SC_OK with motions found
    for name in ("e:257", "c:257:20:22", "far:257:62", "far:512:62"):
        planes, found = inst_ref(pkg, O, name)[3], inst_ref(pkg, O, name)[5]
        assert planes[0]["status"] == SC_OK and found >= 1, (name, _irow(planes, found))
    for mode in (1, 2):
        assert all(inst_ref(pkg, O, name, mode)[5] == MAX_INSTANCES for name in I_MODE_NAMES)   # two inliers' worth passes 4 x 256


def test_the_instances_inside_the_window_are_covariant(pkg, O):
    """records (t times 2^k) and labels for every k inside WIN_REGISTER: what the GPU file's metamorphic check rests on"""
    ks = inst_metamorphic_ks()
    assert len(ks) >= 3
    for n, _ in I_SCENES:
        _, _, _, p0, l0, f0, _ = inst_ref(pkg, O, f"s:{n}:0")
        for k in ks:
            _, _, _, p, l, f, _ = inst_ref(pkg, O, f"s:{n}:{k}")
            assert f == f0 and np.array_equal(l, l0), (n, k)
            for a, b in zip(p, p0):
                assert all(int(a[x]) == int(b[x]) for x in ("status", "n", "edges", "tri_kept", "tri_total", "best_rank", "best_count")), (n, k)
                assert same_bits_nan(a["Rt"][:9], b["Rt"][:9]) and same_bits_nan(a["Rt"][9:], b["Rt"][9:] * pow2(k)), (n, k)
    for mode in (1, 2):                                                         # ... in the truncated modes too
        for n, _ in I_SCENES:
            a, b = (inst_ref(pkg, O, f"s:{n}:{k}", mode) for k in (-56, 62))
            assert _irow(a[3], a[5]) == _irow(b[3], b[5]) and np.array_equal(a[4], b[4]), (mode, n)


def inst_one_launch(pkg, O):
    """All magnitudes under the unit parameters in ONE launch -> (problems, (records, labels, nfound))"""
    if "inst one launch" not in _REF:
        problems = [inst_input(pkg, name)[:2] for name in I_NAMES]
        with np.errstate(**_QUIET):
            _REF["inst one launch"] = (problems, IR.batch(O, problems, dict(UNIT, max_triangles=T), 0, MAX_INSTANCES, min_score_of(0)))
    return _REF["inst one launch"]


def test_the_instances_of_all_magnitudes_in_one_launch(pkg, O):
    problems, (recs, labels, nfound) = inst_one_launch(pkg, O)
    st = recs[0]["status"].tolist()
    print("one launch:", len(st), "problems, found", nfound.tolist(), "status", st)
    assert len(problems) <= 40 and int(recs["tri_total"].max()) <= batch_ref.TRI_CAP
    assert st.count(SC_OK) >= 5 and st.count(SC_ENOHYP) >= 6 and set(nfound.tolist()) == {0, 2, MAX_INSTANCES}
