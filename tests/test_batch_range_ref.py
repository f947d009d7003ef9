"""CPU suite: the inputs of tests/test_gpu_batch_range.py and tests/test_gpu_polish_range.py — sc_register_batch, its slot form
and sc_polish at the ends of the fp32 range — and what the REFERENCE alone says about them.

The two GPU files compare the kernels with tests/batch_ref.py and tests/polish_ref.py bit for bit; that is only worth something if
the inputs really leave the beaten path (other edges, another winner, SC_ENOHYP for the reason meant, every way a polish can
stop) and if no problem is so large that one workgroup runs long.  Both are conditions on the reference, asserted here.

Families (those of tests/test_gpu_range.py, on the scenes of the batch tests: batch_ref.scene(n, rho), T = 200):
  a  coordinates and sigma / tau / min_len times 2^k, k in A_KS, on n = 192, 300, 512;
  b  n = 512 with a block shrunk around the origin (2^-58 with sigma / min_len at its scale; 2^-50 with min_len 0 / subnormal), six
     exact zeros in it; and 64 rows at 2^62 in a unit scene;
  c  n = 300, both clouds 2^20 .. 2^24 from the origin;
  e  n = 300 with rows at +-3e38;
  f  n = 100 with t_cmp / sigma / tau / min_len at the ends of what check_params accepts (test_gpu_range.F_CASES);
  exact100: a complete graph whose keys are all equal — (i, j, k) alone decides the cut; CUTS names the last kept triangle.
"""
import math
from itertools import combinations

import numpy as np
import pytest

import batch_ref
import polish_ref
from test_gpu_range import F_CASES
from test_range_oracle import UNIT, WIN_REGISTER, in_window, pow2, same_bits_nan, scaled, scaled_kw, scene_small, translated

SC_OK, SC_ENOHYP = batch_ref.SC_OK, batch_ref.SC_ENOHYP
T = 200
SCENES = {192: .3, 300: .3, 512: .2}
A_KS = (0, -70, -64, -56, -48, -47, -30, 30, 62, 64, 66, 70)
C_CASES = ("c:20:22", "c:22:24", "c:24:20")
B_CASES = ("b:deep", "b:minlen0", "b:minlen-sub", "b:far62")
# the rows of the n = 512 scene that family b replaces by as many of its first rows, shrunk; B_ZERO: exact zeros among them.
# (128 rows are a clique of C(128, 3) > TRI_CAP triangles in the min_len 0 variants: those take 64 rows, one whole bit word of
# every row)
B_BLOCK = {"deep": slice(256, 384), "minlen0": slice(320, 384), "minlen-sub": slice(320, 384)}
B_ZERO = slice(328, 334)
NAMES = ([f"a:{n}:{k}" for k in A_KS for n in SCENES] + list(C_CASES) + ["e"] + ["f:" + c for c in F_CASES] + list(B_CASES))


def case_kw(name):
    """name -> the parameters of the case's launch (max_triangles included)"""
    fam, *arg = name.split(":")
    kw = dict(UNIT)
    if fam == "a":
        kw = scaled_kw(int(arg[1]))
    elif fam == "b" and arg[0] == "deep":
        kw = scaled_kw(-58, tau=kw["tau"])
    elif fam == "b" and arg[0] != "far62":
        kw["min_len"] = 1e-40 if arg[0] == "minlen-sub" else 0.0
    elif fam == "f":
        kw.update(F_CASES[arg[0]])
    return dict(kw, max_triangles=T)


def case_input(pkg, name):
    """name -> (src, tgt, kw): one problem and the parameters of its launch.  Everything is made of exact operations on seeded scenes."""
    fam, *arg = name.split(":")
    n = {"a": int(arg[0]) if fam == "a" else 0, "b": 512, "c": 300, "e": 300, "f": 100}[fam]
    src, tgt = (x.copy() for x in batch_ref.scene(pkg, n, SCENES.get(n, .3)))
    if fam == "a":
        src, tgt = scaled(src, int(arg[1])), scaled(tgt, int(arg[1]))
    elif fam == "b" and arg[0] == "far62":
        src[64:128] = scaled(src[64:128], 62); tgt[64:128] = scaled(tgt[64:128], 62)
    elif fam == "b":
        blk = B_BLOCK[arg[0]]
        m, sh = blk.stop - blk.start, -58 if arg[0] == "deep" else -50
        src[blk] = scaled(src[:m], sh); tgt[blk] = scaled(tgt[:m], sh)
        src[B_ZERO] = 0; tgt[B_ZERO] = 0
    elif fam == "c":
        src, tgt = translated(src, tgt, int(arg[0]), int(arg[1]))
    elif fam == "e":
        big = np.float32(3e38)
        src[10] = (big, 0, 0); src[70] = (-big, big, 0.1)
        tgt[11] = (0, big, 0); tgt[70] = (big, -big, 0.3); tgt[90] = (-big, -big, -big)
    elif fam != "f":
        raise KeyError(name)
    return src, tgt, case_kw(name)


_REF = {}


def case_ref(pkg, O, name, mode=0):
    """(src, tgt, kw, record, mask) of one case on the reference, once per session; never modified."""
    if (name, mode) not in _REF:
        src, tgt, kw = case_input(pkg, name)
        with np.errstate(over="ignore", under="ignore", divide="ignore"):
            rec, mask = batch_ref.one(O, src, tgt, kw, mode)
        _REF[name, mode] = (src, tgt, kw, rec, mask)
    return _REF[name, mode]


def groups(names=NAMES):
    """The cases packed by parameter set (a launch has one sc_params): [(kw, [name, ...]), ...] in first-seen order."""
    out = {}
    for name in names:
        kw = case_kw(name)
        out.setdefault(tuple(sorted(kw.items())), (kw, []))[1].append(name)
    return list(out.values())


def _row(rec):
    return tuple(int(rec[f]) for f in ("status", "edges", "tri_total", "tri_kept", "best_rank", "best_count"))


# ---- the record of every case, as the reference gives it -------------------------------------------------------------------------
# (edges, rank, count) of family a — whoever changes a scene or a parameter sees here what the GPU file then no longer covers
A_EXPECT = {(192, -70): (1619, 82, 43), (300, -70): (4421, 181, 73), (512, -70): (8548, 70, 77),
            (192, 0): (1624, 77, 52), (300, 0): (4416, 18, 85), (512, 0): (8532, 14, 101)}


def test_every_problem_stays_under_the_cap(pkg, O):
    """A workgroup's run time is (triangles of the graph) x passes: no case holds more than batch_ref.TRI_CAP."""
    worst = ("", 0)
    for name in NAMES:
        rec = case_ref(pkg, O, name)[3]
        print(name, _row(rec))
        worst = max(worst, (name, int(rec["tri_total"])), key=lambda x: x[1])
        assert int(rec["tri_total"]) <= batch_ref.TRI_CAP, name
    print("largest:", worst)


def test_family_a_differs_from_unit_scale(pkg, O):
    """Outside the windows the graph, the winner and its count are really other ones than at k = 0; at k = 66 the list is shorter
    than T (no selection runs); at k = 70 nothing is left."""
    for n in SCENES:
        r0 = case_ref(pkg, O, f"a:{n}:0")[3]
        assert r0["status"] == SC_OK and (int(r0["edges"]), int(r0["best_rank"]), int(r0["best_count"])) == A_EXPECT[n, 0]
        assert int(r0["tri_total"]) > T
        for k in (-70, -64, 64):
            r = case_ref(pkg, O, f"a:{n}:{k}")[3]
            assert r["status"] == SC_OK, (n, k)
            assert (int(r["best_rank"]), int(r["best_count"])) != (int(r0["best_rank"]), int(r0["best_count"])), (n, k)
        r = case_ref(pkg, O, f"a:{n}:-70")[3]
        assert (int(r["edges"]), int(r["best_rank"]), int(r["best_count"])) == A_EXPECT[n, -70]
        assert int(case_ref(pkg, O, f"a:{n}:64")[3]["edges"]) < int(r0["edges"])
        r = case_ref(pkg, O, f"a:{n}:66")[3]
        assert r["status"] == SC_OK and 0 < int(r["tri_total"]) < T and int(r["tri_kept"]) == int(r["tri_total"]), (n, _row(r))
        r = case_ref(pkg, O, f"a:{n}:70")[3]
        assert (int(r["status"]), int(r["edges"])) == (SC_ENOHYP, 0), n
    assert [int(case_ref(pkg, O, f"a:{n}:-64")[3]["best_rank"]) for n in SCENES] == [130, 107, 19]
    assert [int(case_ref(pkg, O, f"a:{n}:64")[3]["edges"]) for n in SCENES] == [1527, 4035, 7695]
    assert [int(case_ref(pkg, O, f"a:{n}:66")[3]["tri_total"]) for n in SCENES] == [7, 67, 79]


def test_family_a_inside_the_window_is_covariant_on_these_scenes(pkg, O):
    """What the GPU file's metamorphic check (the GPU at k against the GPU at k = 0) rests on: the windows of test_range_oracle.py
    were derived for unit scenes, and the batch scenes are such."""
    for n in SCENES:
        s0, t0, _, r0, m0 = case_ref(pkg, O, f"a:{n}:0")
        assert max(np.ptp(s0, axis=0).max(), np.ptp(t0, axis=0).max()) < 3.0
        for k in metamorphic_ks():
            _, _, _, r, m = case_ref(pkg, O, f"a:{n}:{k}")
            assert _row(r) == _row(r0) and np.array_equal(m, m0), (n, k)
            assert same_bits_nan(r["Rt"][:9], r0["Rt"][:9]) and same_bits_nan(r["Rt"][9:], r0["Rt"][9:] * pow2(k)), (n, k)


def metamorphic_ks():
    return [k for k in A_KS if k and in_window(k, WIN_REGISTER)]


def test_the_other_families_are_what_they_are_used_for(pkg, O):
    """Statuses and the counts that say WHY: SC_ENOHYP without an edge, SC_ENOHYP after scoring (f:tau-30: 200 hypotheses, no
    inlier — the k0 == 0 exit), every point an inlier (f:tau25), every key equal and the cut among them (f:sigma30).

    Family b on the reference (edges / triangles / kept / rank / count), all SC_OK:
      b:deep         616 /   1 331 / 200 /   0 / 128   the 128-row block's own graph (sigma, min_len = 2^-58 x 0.05: nothing else is an
                                                        edge), and at the unit tau the whole block is every hypothesis' inlier
      b:minlen0     9763 / 125 436 / 200 / 197 /  66   64 rows (128 would be a clique of 341 376 triangles, over the cap): every pair
                                                        of the block has weight 1 — C(64, 3) = 41 664 equal keys on top, the cut among them
      b:minlen-sub  9748 / 124 246 / 200 / 197 /  66   the 15 pairs among the six zeros are no edges: 0 < 1e-40
      b:far62       6359 /  39 739 / 200 /  47 /  86
    """
    rows = {name: _row(case_ref(pkg, O, name)[3]) for name in NAMES if not name.startswith("a:")}
    for name, row in rows.items():
        print(name, row)
    ok = ["c:20:22", "e", "f:tcmp38", "f:tcmp44", "f:sigma30", "f:tau25", "f:minlen-sub"] + list(B_CASES)
    no_edge = ["c:22:24", "c:24:20", "f:tcmp1", "f:sigma-30", "f:minlen38"]
    assert all(rows[c][0] == SC_OK and rows[c][1] > 0 for c in ok), [c for c in ok if rows[c][0] != SC_OK]
    assert all(rows[c][:2] == (SC_ENOHYP, 0) for c in no_edge), [c for c in no_edge if rows[c][:2] != (SC_ENOHYP, 0)]
    assert rows["c:20:22"][2] == 420
    assert (rows["e"][2], rows["e"][5]) == (40804, 84)
    assert rows["f:tau-30"] == (SC_ENOHYP, 523, 1826, 200, 0, 0)
    assert rows["f:tau25"] == (SC_OK, 523, 1826, 200, 0, 100)
    assert rows["f:sigma30"] == (SC_OK, 4944, 161112, 200, 100, 3)
    assert (rows["f:tcmp38"][2], rows["f:tcmp44"][2]) == (128507, 137115)
    assert rows["b:deep"] == (SC_OK, 616, 1331, 200, 0, 128)
    assert rows["b:minlen0"] == (SC_OK, 9763, 125436, 200, 197, 66)
    assert rows["b:minlen-sub"] == (SC_OK, 9748, 124246, 200, 197, 66) and rows["b:minlen0"][1] - rows["b:minlen-sub"][1] == math.comb(6, 2)
    assert rows["b:far62"] == (SC_OK, 6359, 39739, 200, 47, 86)
    assert math.comb(B_BLOCK["minlen0"].stop - B_BLOCK["minlen0"].start, 3) == 41664 < rows["b:minlen-sub"][2]


def test_all_magnitudes_in_one_launch_stay_under_the_cap(pkg, O):
    """The GPU file also packs every case's points into ONE batch under the unit parameters (a launch has one parameter set):
    workgroups next to each other at 2^-70 .. 2^70, +-3e38 and 2^24 from the origin.  Its reference, and that it is not trivial."""
    recs, _ = one_launch_ref(pkg, O)
    assert int(recs["tri_total"].max()) <= batch_ref.TRI_CAP
    st = recs["status"].tolist()
    print("one launch:", len(st), "problems,", st.count(SC_OK), "SC_OK,", st.count(SC_ENOHYP), "SC_ENOHYP")
    assert st.count(SC_OK) >= 8 and st.count(SC_ENOHYP) >= 10


# (family f is the unit scene: its parameters are what differs; eight of family a's k: at most 40 workgroups a launch)
ONE_LAUNCH = [name for name in NAMES if not name.startswith("f:") and not (name.startswith("a:") and int(name.split(":")[2]) in (-64, -48, -47, 66))]


def one_launch_problems(pkg):
    return [case_input(pkg, name)[:2] for name in ONE_LAUNCH]


def one_launch_ref(pkg, O):
    if "one launch" not in _REF:
        with np.errstate(over="ignore", under="ignore", divide="ignore"):
            _REF["one launch"] = batch_ref.batch(O, one_launch_problems(pkg), dict(UNIT, max_triangles=T))
    return _REF["one launch"]


# ---- the cut among equal keys -------------------------------------------------------------------------------------------------
EXACT_N = 100
EXACT_TOTAL = math.comb(EXACT_N, 3)


def exact100():
    """100 points on the grid integers(-512, 512) / 64, tgt = src + (2, -1, 0.5) (batch_ref.exact_scene at n = 100): two words a
    row, 7 column chunks.  The graph is complete and every key equal in both rank modes."""
    rng = np.random.default_rng(41)
    src = (rng.integers(-512, 512, size=(EXACT_N, 3)) / 64).astype(np.float32)
    return src, (src + np.array([2, -1, 0.5], np.float32)).astype(np.float32)


def position(i, j, k, n=EXACT_N):
    """1 + the triangles of the complete graph on n vertices before (i, j, k) in ascending lexicographic order: the T at which
    (i, j, k) is the last one kept."""
    rows = sum((n - 1 - a) * (n - 2 - a) // 2 for a in range(i))      # rows a < i: C(n - 1 - a, 2) each
    edges = sum(n - 1 - b for b in range(i + 1, j))                   # edges (i, b), b < j: n - 1 - b each
    return rows + edges + (k - j - 1) + 1


CUT_TRIANGLES = {}                                                     # name -> the last triangle kept
for _i, _j in ((3, 40), (20, 62)):
    for _k in (63, 64, 65):                                           # k at / across bit 63 | 64 of a two-word row
        CUT_TRIANGLES[f"({_i},{_j},{_k})"] = (_i, _j, _k)
for _t in ((3, 63, 64), (3, 63, 99), (3, 64, 65), (62, 63, 64), (63, 64, 65)):   # j, and the row, at / across the word boundary
    CUT_TRIANGLES[str(_t).replace(" ", "")] = _t
for _i in (3, 4, 63, 64):                                             # the last triangle of a row (an even row: need == pre + v0)
    CUT_TRIANGLES[f"last of row {_i}"] = (_i, 98, 99)
for _i in (4, 5, 64):                                                 # the first triangle of a row (rem == 1 in the j pass)
    CUT_TRIANGLES[f"first of row {_i}"] = (_i, _i + 1, _i + 2)
for _j in (15, 16, 79, 80):                                           # j at the edge of a 16-column chunk
    CUT_TRIANGLES[f"first of edge (2,{_j})"] = (2, _j, _j + 1)         # (rem == 1 in the k pass)
    CUT_TRIANGLES[f"last of edge (2,{_j})"] = (2, _j, 99)
CUTS = {name: position(*t) for name, t in CUT_TRIANGLES.items()}      # name -> T
CUTS.update({"T=1": 1, "T=total-1": EXACT_TOTAL - 1, "T=total": EXACT_TOTAL, "T=total+1": EXACT_TOTAL + 1})

# On exact100 every hypothesis is the same translation: the winner is (0, 1, 2) with all 100 inliers wherever the cut falls, and a
# cut one triangle off shows nowhere in the record.  cut_scene makes the triangle AT the cut the winner: the points of H = {i, j,
# k, k + 1, ..} keep the translation, every other target point is moved by its own offset from {-1, 0, 1}^3 / 256 (exact on the
# grid; any two offsets differ by less than d_thr = 0.0229, so the graph stays complete and under SC_RANK_DEGREE every key equal),
# and tau = 0.0002 << 1 / 256 tells the offsets apart.  (i, j, k) is the first triangle inside H in ascending order: kept, it wins
# with |H| inliers at rank T - 1; cut off, something else wins.
# A cut whose last triangle ends a row or an edge (k = 99: H would be three points) is run on the scene of its SUCCESSOR, at the
# successor's T - 1: one triangle too many and the successor wins.
CUT_KW = dict(UNIT, tau=0.0002, rank_mode=1)
CUT_MIN_H = 20


def successor(i, j, k, n=EXACT_N):
    return (i, j, k + 1) if k + 1 < n else (i, j + 1, j + 2) if j + 2 < n else (i + 1, i + 2, i + 3)


def cut_winner(name):
    """the triangle whose scene the cut `name` runs on: its own last triangle, or that one's successor"""
    t = CUT_TRIANGLES[name]
    return t if t[2] < EXACT_N - 1 else successor(*t)


def cut_scene(i, j, k):
    src, tgt = exact100()
    rng = np.random.default_rng(1000 * i + 10 * j + k)
    h = np.zeros(EXACT_N, bool)
    h[[i, j]] = True; h[k:] = True
    off = rng.integers(-1, 2, size=(EXACT_N, 3))
    zero = ~off.any(1)
    off[zero, 0] = 1                                                  # no offset is (0, 0, 0) outside H
    off[h] = 0
    return src, (tgt + (off / 256).astype(np.float32)).astype(np.float32), int(h.sum())


_CUT_SCENE_REF = {}


def cut_scene_ref(O, name):
    """-> (problem, |H|, T of cut_winner(name), reference at T, reference at T - 1); CUTS[name] is T or T - 1"""
    if name not in _CUT_SCENE_REF:
        src, tgt, nh = cut_scene(*cut_winner(name))
        T_ = position(*cut_winner(name))
        assert CUTS[name] in (T_, T_ - 1)
        _CUT_SCENE_REF[name] = ((src, tgt), nh, T_, batch_ref.batch(O, [(src, tgt)], dict(CUT_KW, max_triangles=T_)),
                                batch_ref.batch(O, [(src, tgt)], dict(CUT_KW, max_triangles=T_ - 1)))
    return _CUT_SCENE_REF[name]


@pytest.mark.parametrize("name", list(CUT_TRIANGLES))
def test_the_triangle_at_the_cut_wins_when_it_is_kept(O, name):
    (src, tgt), nh, T_, at, before = cut_scene_ref(O, name)
    r, r1 = at[0][0], before[0][0]
    print(name, "|H|", nh, "T", T_, _row(r), "| T - 1:", _row(r1))
    assert (int(r["status"]), int(r["edges"]), int(r["tri_total"]), int(r["tri_kept"])) == (SC_OK, 4950, EXACT_TOTAL, T_)
    assert (int(r1["status"]), int(r1["tri_total"]), int(r1["tri_kept"])) == (SC_OK, EXACT_TOTAL, T_ - 1)
    assert nh >= CUT_MIN_H
    assert (int(r["best_rank"]), int(r["best_count"])) == (T_ - 1, nh) and at[1][0].sum() == nh
    assert int(r1["best_count"]) < nh and int(r1["best_rank"]) < T_ - 1


def test_position_is_the_rank_in_lexicographic_order():
    for n in (7, 100):
        for pos, (i, j, k) in enumerate(combinations(range(n), 3), start=1):
            assert position(i, j, k, n) == pos, (n, i, j, k)
    assert position(97, 98, 99) == EXACT_TOTAL and position(0, 1, 2) == 1
    assert len(set(CUTS.values())) == len(CUTS)
    assert position(3, 98, 99) + 1 == position(4, 5, 6)               # last of row 3 / first of row 4: neighbours


@pytest.mark.parametrize("rank_mode", [0, 1])
def test_exact100_is_a_complete_graph_of_equal_keys(O, rank_mode):
    src, tgt = exact100()
    S, bits, deg = O.compat(src, tgt, UNIT["sigma"], UNIT["t_cmp"], UNIT["min_len"], UNIT["tau"])
    assert int(deg.sum()) // 2 == 4950 and (deg == 99).all() and (S[~np.eye(100, dtype=bool)] == 1).all()
    tri, key, total = O.triangles(S, bits, deg, EXACT_TOTAL, rank_mode)
    assert total == EXACT_TOTAL == 161700 and len(np.unique(key >> np.uint64(32) if key.dtype == np.uint64 else key)) >= 1
    assert np.array_equal(tri, np.array(list(combinations(range(100), 3)), tri.dtype))      # ... kept in ascending (i, j, k)
    for what in ("(3,40,64)", "last of row 4", "T=total-1"):
        rec, mask = batch_ref.one(O, src, tgt, dict(UNIT, max_triangles=CUTS[what], rank_mode=rank_mode))
        assert (int(rec["status"]), int(rec["tri_total"]), int(rec["tri_kept"]), int(rec["best_rank"]), int(rec["best_count"])) == \
               (SC_OK, EXACT_TOTAL, CUTS[what], 0, 100), what
        assert mask.all()


# ---- sc_polish ----------------------------------------------------------------------------------------------------------------
POLISH_T, POLISH_K, POLISH_ITERS = 2000, 8, 16
POLISH_KS = (0, -64, -56, -48, -30, 30, 62, 64)
POLISH_CASES = ([f"a:{k}" for k in POLISH_KS] + ["c:20:22", "e", "f:tau-30", "f:tau25", "a:-56:mode1", "a:-56:mode2", "a:62:mode1", "a:62:mode2",
                                                 "sparse:-40", "sparse:40"])


def polish_k(name):
    return 64 if name.startswith("sparse") else POLISH_K


def polish_input(pkg, name):
    """name -> (src, tgt, kw, score_mode) on test_range_oracle.scene_small (n = 300), T = 2000; sparse: polish_ref.sparse_scene
    times 2^k with 64 candidates asked for (fewer exist, and refits are declined before the first: fewer than three inliers)."""
    fam, *arg = name.split(":")
    mode = int(arg[-1][4:]) if arg and arg[-1].startswith("mode") else 0
    if fam == "sparse":
        kw, src, tgt = polish_ref.sparse_scene(pkg)
        k = int(arg[0])
        return scaled(src, k), scaled(tgt, k), scaled_kw(k, base=kw), mode
    src, tgt = scene_small(pkg)
    kw = dict(UNIT)
    if fam == "a":
        k = int(arg[0])
        src, tgt, kw = scaled(src, k), scaled(tgt, k), scaled_kw(k)
    elif fam == "c":
        src, tgt = translated(src, tgt, int(arg[0]), int(arg[1]))
    elif fam == "e":
        big = np.float32(3e38)
        src[10] = (big, 0, 0); src[70] = (-big, big, 0.1)
        tgt[11] = (0, big, 0); tgt[70] = (big, -big, 0.3); tgt[90] = (-big, -big, -big)
    elif fam == "f":
        kw.update(F_CASES[arg[0]])
    else:
        raise KeyError(name)
    return src, tgt, dict(kw, max_triangles=POLISH_T), mode


def polish_case_ref(pkg, O, name):
    """(src, tgt, kw, mode, frame: the restatement's whole path, hyp: polish_ref.hypotheses, exp: polish_ref.polish), once."""
    if ("polish", name) not in _REF:
        src, tgt, kw, mode = polish_input(pkg, name)
        th = min(O.max_threads(), 8)
        with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
            frame = O.register(src, tgt, threads=th, score_mode=mode, **kw)
            hyp = polish_ref.hypotheses(O, src, tgt, kw, th)
            exp = polish_ref.polish(O, src, tgt, hyp["Rt"], kw["tau"], mode, polish_k(name), POLISH_ITERS, threads=th) if len(hyp["Rt"]) else None
        _REF["polish", name] = (src, tgt, kw, mode, frame, hyp, exp)
    return _REF["polish", name]


def test_the_polish_cases_stop_in_every_way(pkg, O):
    """Per case how each candidate stopped on the reference; the set holds a fixed point, a declined refit, a candidate that was
    refitted at least twice, a frame without a candidate (f:tau-30) and one whose every point is every candidate's inlier."""
    stops, most = set(), 0
    for name in POLISH_CASES:
        src, tgt, kw, mode, frame, hyp, exp = polish_case_ref(pkg, O, name)
        cand = exp["cand"] if exp else []
        print(name, "frame", frame["rc"], "t_eff", frame["t_eff"], "rank", frame["best_rank"], "count", frame["best_count"], "| polish",
              exp["status"] if exp else None, [(c["rank"], c["score0"], c["score"], c["iters"], c["stop"]) for c in cand])
        stops |= {c["stop"] for c in cand}
        most = max([most] + [c["iters"] for c in cand])
        if name == "f:tau-30":
            assert frame["rc"] == -5 and frame["t_eff"] == POLISH_T and exp["status"] == SC_ENOHYP and not cand
        elif name == "f:tau25":
            assert exp["status"] == SC_OK and all(c["score0"] == len(src) for c in cand) and len(cand) == POLISH_K
        elif name.startswith("sparse"):
            assert 0 < len(cand) < 64 and any(c["stop"] == "declined" and c["iters"] == 0 for c in cand), name
        else:
            assert frame["rc"] == 0 and exp["status"] == SC_OK and cand, name
            assert frame["best_rank"] == cand[0]["rank"] and frame["best_count"] == cand[0]["score0"], name   # the frame's winner comes first
    assert {"fixed", "declined", "max_iter"} <= stops and most >= 2, (stops, most)
    far = polish_case_ref(pkg, O, "c:20:22")[6]["cand"]        # a refit declined after refits that were not: the iterate lost its inliers
    assert any(c["stop"] == "declined" and c["iters"] > 0 for c in far)


def test_polish_inside_the_window_is_covariant(pkg, O):
    """What the GPU file's metamorphic check of sc_polish rests on."""
    e0 = polish_case_ref(pkg, O, "a:0")[6]
    for k in polish_metamorphic_ks():
        e = polish_case_ref(pkg, O, f"a:{k}")[6]
        assert [(c["rank"], c["score0"], c["score"], c["iters"], c["stop"]) for c in e["cand"]] == \
               [(c["rank"], c["score0"], c["score"], c["iters"], c["stop"]) for c in e0["cand"]], k
        for c, c0 in zip(e["cand"], e0["cand"]):
            assert same_bits_nan(c["Rt"][:9], c0["Rt"][:9]) and same_bits_nan(c["Rt"][9:], c0["Rt"][9:] * pow2(k)), k
        assert np.array_equal(e["mask"], e0["mask"]) and e["winner"] == e0["winner"], k


def polish_metamorphic_ks():
    return [k for k in POLISH_KS if k and in_window(k, WIN_REGISTER)]
