"""CPU suite: the surface of sc_pairs_cycles (include/saccot.h) — the four exports, the Python mirror, the layouts of
sc_cycle_params, sc_cycle_result and sc_cycle_summary compiled in C99, the default parameters, sc_cycles_thresholds, every rule that
refuses a call with its text (the host-only rules and the adjacency build run under the sanitizers, in a program of their own) — and
the Python restatement (tests/cycles_ref.py) that the GPU tests compare against: its input families are checked for what they are
used for.  No compute call reaches a GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import cycles_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_cycles_default_params", "sc_cycles_thresholds", "sc_pairs_cycles", "sc_pairs_cycles_device")
SC_OK, SC_EINVAL = 0, -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def _section():
    header = _header()
    return header[header.index("sc_pairs_cycles ---"):header.index("sc_match_guided_poses ---")]


def test_cycles_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    for method in ("pairs_cycles", "pairs_cycles_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert callable(pkg.make_cycle_params) and callable(pkg.cycles_thresholds)
    for struct, dtype, ref in (("ScCycleResult", "CYCLE_RESULT_DTYPE", CR.RESULT_DTYPE), ("ScCycleSummary", "CYCLE_SUMMARY_DTYPE", CR.SUMMARY_DTYPE)):
        S, D = getattr(pkg, struct), getattr(pkg, dtype)
        assert np.dtype(S) == D and D.itemsize == C.sizeof(S) == ref.itemsize and list(D.names) == list(ref.names)
        assert [D.fields[f][1] for f in D.names] == [ref.fields[f][1] for f in ref.names] == [getattr(S, f).offset for f in D.names]
        assert [D.fields[f][0] for f in D.names] == [ref.fields[f][0] for f in ref.names]
    assert (pkg.SC_CYCLES_STATUS, pkg.SC_CYCLES_MAX_PAIRS, pkg.SC_CYCLES_MAX_DEGREE, CR.STATUS) == (1, 1 << 22, 65535, 1)


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_PAIRS_CYCLES 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_the_section_says_what_is_not_here_and_states_every_rule():
    block = _section()
    flat = " ".join(block.replace("\n * ", "\n").split())  # (the comment's line starts taken out; a product's " * " stays)
    for word in ("Not here:", "solving the pose graph", "loops longer than three", "information matrices", "a sharded form"):
        assert word in flat
    for rule in ("tr_min = 1.0 + 2.0 * cos((double)rot_tol)", "e2_max = (double)trans_tol * (double)trans_tol",
                 "t'_c = -((R_0c * t_0 + R_1c * t_1) + R_2c * t_2)",
                 "M.R_ij = ((B.R_i0 * A.R_0j + B.R_i1 * A.R_1j) + B.R_i2 * A.R_2j)",
                 "M.t_i = ((B.R_i0 * A.t_0 + B.R_i1 * A.t_1) + B.R_i2 * A.t_2) + B.t_i",
                 "E = T_r(c->a) o (T_q(b->c) o T_p(a->b))", "tr = (E.R_00 + E.R_11) + E.R_22",
                 "e2 = (E.t_0 * E.t_0 + E.t_1 * E.t_1) + E.t_2 * E.t_2", "tr >= tr_min && e2 <= e2_max",
                 "alive_k(p) = alive_{k-1}(p) && (ok_k(p) >= min_ok || keep[p])"):
        assert rule in flat, rule
    # what finite poses can and cannot do to the chains, and the half turn
    for claim in ("both cuts inclusive", "No NaN arises from finite fp32 poses", "tr cannot overflow", "e2 itself may overflow to +inf with hostile finite poses",
                  "+inf is then the largest max_e2 there is, and it is never consistent", "A loop off by exactly a half turn (tr = -1) is not consistent at any rot_tol",
                  "tr_min = -1 + 7.5e-15"):
        assert claim in flat, claim
    assert "cannot overflow these chains" not in flat
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "2f-1" in integration and "sc_pairs_cycles_device" in integration


def test_the_struct_layouts_and_the_macros_in_c(pkg, tmp_path):
    exe = str(tmp_path / "cycles_layout")
    P, R, S = "sc_cycle_params", "sc_cycle_result", "sc_cycle_summary"
    pf = ("size", "min_ok", "max_rounds", "flags", "rot_tol", "trans_tol", "reserved")
    rf = ("status", "cycles", "ok", "ok_alive", "alive", "dropped_round", "min_trace", "max_e2", "reserved")
    sf = ("rounds", "stable", "alive", "edges", "triangles", "consistent")
    fields = ([f"sizeof({P})"] + [f"offsetof({P}, {f})" for f in pf] + [f"sizeof({R})"] + [f"offsetof({R}, {f})" for f in rf]
              + [f"sizeof({S})"] + [f"offsetof({S}, {f})" for f in sf])
    consts = ["SC_CYCLES_STATUS", "SC_CYCLES_MAX_PAIRS", "SC_CYCLES_MAX_DEGREE", "SC_HAS_PAIRS_CYCLES"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("' + "%zu " * len(fields) + "%u " * len(consts)
           + '", ' + ", ".join(fields) + ", " + ", ".join(f"(unsigned){c}" for c in consts) + ");return 0;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[:8] == [32, 0, 4, 8, 12, 16, 20, 24] == [C.sizeof(pkg.ScCycleParams)] + [getattr(pkg.ScCycleParams, f).offset for f in pf]
    assert got[8:18] == [48, 0, 4, 8, 12, 16, 20, 24, 32, 40] == [C.sizeof(pkg.ScCycleResult)] + [getattr(pkg.ScCycleResult, f).offset for f in rf]
    assert got[18:25] == [32, 0, 4, 8, 12, 16, 24] == [C.sizeof(pkg.ScCycleSummary)] + [getattr(pkg.ScCycleSummary, f).offset for f in sf]
    assert got[25:] == [1, 1 << 22, 65535, 1]


def test_default_params_and_null_arguments(pkg):
    L = pkg.load_library()
    cp = pkg.ScCycleParams()
    cp.reserved[1] = 9; cp.rot_tol = 0.5; cp.flags = 1
    assert L.sc_cycles_default_params(C.byref(cp)) == SC_OK
    assert (cp.size, cp.min_ok, cp.max_rounds, cp.flags, cp.rot_tol, cp.trans_tol, list(cp.reserved)) == (32, 1, 16, 0, 0.0, 0.0, [0, 0])
    assert L.sc_cycles_default_params(None) == SC_EINVAL
    assert bytes(pkg.make_cycle_params(0.0, 0.0)) == bytes(cp)  # the Python defaults are the library's
    mk = pkg.make_cycle_params(0.25, 0.5, min_ok=3, max_rounds=7, flags=1)
    assert (mk.size, mk.min_ok, mk.max_rounds, mk.flags, mk.rot_tol, mk.trans_tol) == (32, 3, 7, 1, 0.25, 0.5)
    # (a context cannot exist here — sc_create fails without a GPU — so the NULL context is what is tried; the GPU suite tries the
    # rest with a context and reads sc_last_error, and the program below checks every rule's text)
    pairs = (C.c_uint32 * 2)(0, 1)
    assert L.sc_pairs_cycles(None, 2, pairs, 1, C.byref(mk), None, 48, None, None, None) == SC_EINVAL
    assert L.sc_pairs_cycles_device(None, 2, pairs, 1, C.byref(mk), None, 48, None, None, None) == SC_EINVAL


def _ulps(a, b):
    ka, kb = (int(np.array(x, np.float64).view(np.int64)) for x in (a, b))
    return abs(ka - kb)


def test_the_thresholds(pkg):
    L = pkg.load_library()
    out = (C.c_double * 2)()
    for rot, trans in ((0.0, 0.0), (math.radians(0.5), 0.01), (0.25, 0.5), (1.0, 3.0), (math.pi / 2, 1e-3), (3.1415927, 1e19), (1e-4, 1e-20)):
        cp = pkg.make_cycle_params(rot, trans)
        assert L.sc_cycles_thresholds(C.byref(cp), out) == SC_OK
        rot32, trans32 = float(np.float32(rot)), float(np.float32(trans))
        want_c = math.cos(rot32)
        # the library's cos may differ from Python's by a unit in the last place: tr_min = 1 + 2 cos within 4 ulp of it, and the
        # square exactly
        assert _ulps(out[0], 1.0 + 2.0 * want_c) <= 4, (rot, out[0], 1.0 + 2.0 * want_c)
        assert out[1] == trans32 * trans32
        assert pkg.cycles_thresholds(cp) == (out[0], out[1])
    assert L.sc_cycles_thresholds(None, out) == SC_EINVAL and L.sc_cycles_thresholds(C.byref(cp), None) == SC_EINVAL
    for bad in (pkg.make_cycle_params(-0.1, 0.0), pkg.make_cycle_params(3.2, 0.0), pkg.make_cycle_params(0.1, -1.0),
                pkg.make_cycle_params(float("nan"), 0.0), pkg.make_cycle_params(0.1, float("inf")), pkg.make_cycle_params(0.1, 0.1, max_rounds=65)):
        assert L.sc_cycles_thresholds(C.byref(bad), out) == SC_EINVAL
    wrong = pkg.make_cycle_params(0.1, 0.1); wrong.size = 28
    assert L.sc_cycles_thresholds(C.byref(wrong), out) == SC_EINVAL


def test_the_host_rules_and_the_adjacency_under_the_sanitizers(tmp_path):
    """Every refusal rule of sc_cycles_check.hpp with its text, the thresholds, and the adjacency of lists with self pairs, repeats,
    both directions, an unreferenced set and a degree of exactly 65 535 / 65 536: tests/native/cycles_check_main.cpp, a program of
    its own built with -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "cycles_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "cycles_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


# ---- the reference itself: the families are what they are used for ----------------------------------------------------------------
def _thr(f):
    return 1.0 + 2.0 * math.cos(float(np.float32(f.params["rot_tol"]))), float(np.float32(f.params["trans_tol"])) ** 2


def test_k24_is_what_it_is_used_for():
    f = CR.k24()
    assert f.n_sets == 24 and len(f.pairs) == 276 and len(f.bad) == 28
    assert len({(min(a, b), max(a, b)) for a, b in f.pairs.tolist()}) == 276
    assert 60 < (f.pairs[:, 0] > f.pairs[:, 1]).sum() < 216 and (np.diff(f.pairs.min(axis=1).astype(np.int64)) < 0).any()  # directions, order
    clean = np.ones(276, bool); clean[f.bad] = False
    for min_ok in (1, 3, 8):
        res, s = CR.cycles(24, f.pairs, f.rt, *_thr(f), min_ok=min_ok)
        print(min_ok, s, "ok of the clean pairs", res["ok"][clean].min(), res["ok"][clean].max(), "min_trace", res["min_trace"].min(), "max_e2", res["max_e2"].max())
        assert (s["triangles"], s["consistent"], s["edges"]) == (2024, 1476, 276)
        assert (res["cycles"] == 22).all() and (res["ok"][clean] >= 12).all() and (res["ok"][f.bad] == 0).all()
        assert (s["rounds"], s["stable"], s["alive"]) == (2, 1, 248)
        assert (res["alive"][clean] == 1).all() and (res["alive"][f.bad] == 0).all() and (res["dropped_round"][f.bad] == 1).all()
        assert (res["dropped_round"][clean] == 0).all() and (res["ok_alive"][f.bad] == 0).all()
        assert (res["ok_alive"][clean] == res["ok"][clean]).all()  # (no clean pair's consistent loop held a corrupted pair)
        assert (res["status"] == SC_OK).all() and not res["reserved"].any()
    # the extrema are the arithmetic's: a clean loop's trace is 3 but for the rounding, a corrupted one's is far below
    assert res["min_trace"][f.bad].max() < 1.0 + 2.0 * math.cos(math.radians(4.9)) and res["max_e2"][clean].max() > 0.0
    # the order of the list does not matter: the records permute
    perm = np.random.default_rng(3).permutation(276)
    res2, s2 = CR.cycles(24, f.pairs[perm], f.rt[perm], *_thr(f), min_ok=3)
    res3, s3 = CR.cycles(24, f.pairs, f.rt, *_thr(f), min_ok=3)
    assert res2.tobytes() == res3[perm].tobytes() and s2.tobytes() == s3.tobytes()


def test_the_strip_unravels_a_pair_a_round():
    f = CR.strip()
    assert f.n_sets == 42 and len(f.pairs) == 81 and f.keep.sum() == 41
    res, s = CR.cycles(42, f.pairs, f.rt, *_thr(f), min_ok=2, max_rounds=64, keep=f.keep)
    assert (s["triangles"], s["consistent"], s["rounds"], s["stable"], s["alive"], s["edges"]) == (40, 40, 41, 1, 41, 81)
    assert res["dropped_round"][:40].tolist() == list(range(1, 41)) and not res["dropped_round"][40:].any()
    assert res["alive"][40:].all() and res["ok_alive"][40] == 0 and res["ok"][40] == 1  # the protected chain pair closes nothing in the end
    res, s = CR.cycles(42, f.pairs, f.rt, *_thr(f), min_ok=2, max_rounds=5, keep=f.keep)
    assert (s["rounds"], s["stable"], s["alive"]) == (5, 0, 76) and (res["dropped_round"] > 0).sum() == 5
    assert res["dropped_round"][:6].tolist() == [1, 2, 3, 4, 5, 0] and res["ok_alive"][4] == 1  # ok_K of the pair the last round dropped
    res, s = CR.cycles(42, f.pairs, f.rt, *_thr(f), min_ok=0, keep=None)
    assert (s["rounds"], s["stable"], s["alive"]) == (1, 1, 81) and not res["dropped_round"].any()


def test_the_other_families():
    f = CR.hub()
    assert f.n_sets == 1500 and (f.pairs == 0).any(axis=1).sum() == 1499
    res, s = CR.cycles(f.n_sets, f.pairs, f.rt, *_thr(f))
    assert s["triangles"] == 1498 and 0 < s["consistent"] < 1498 and s["stable"] == 1 and 0 < s["alive"] < s["edges"] == len(f.pairs)
    assert (res["alive"][f.bad] == 0).all()
    f = CR.k24_repeats()
    res, s = CR.cycles(24, f.pairs, f.rt, *_thr(f))
    assert len(f.pairs) == 283 and s["triangles"] > 2024 and res["cycles"].max() > 22 and (res["alive"][f.bad] == 0).all() and s["alive"] == 283 - 28
    for directions in range(8):
        for consistent in (True, False):
            f = CR.one_triangle(directions, consistent)
            res, s = CR.cycles(3, f.pairs, f.rt, *_thr(f))
            assert (s["triangles"], s["consistent"], s["alive"]) == (1, int(consistent), 3 if consistent else 0)
            assert res["cycles"].tolist() == [1, 1, 1] and len(set(res["min_trace"].tolist())) == 1 and len(set(res["max_e2"].tolist())) == 1
    # invalid pairs and self pairs take part in nothing
    f = CR.k24()
    rt = f.rt.copy(); rt[5, 3] = np.nan
    st = np.zeros(276, np.int32); st[9] = -5
    pairs = f.pairs.copy(); pairs[11] = (7, 7)
    res, s = CR.cycles(24, pairs, rt, *_thr(f), statuses=st)
    assert res["status"][[5, 9, 11]].tolist() == [SC_EINVAL, -5, SC_OK] and s["edges"] == 273
    assert not res[[5, 9, 11]]["cycles"].any() and not res[[5, 9, 11]]["alive"].any() and (res["min_trace"][[5, 9, 11]] == 3.0).all()
    others = np.setdiff1d(np.arange(276), [5, 9, 11])
    alone = CR.cycles(24, pairs[others], rt[others], *_thr(f))
    assert res[others].tobytes() == alone[0].tobytes()


# ---- the families of the range tests (tests/test_gpu_pairs_cycles_range.py) -----------------------------------------------------------
def _cut(rot_tol, trans_tol):
    return 1.0 + 2.0 * math.cos(float(np.float32(rot_tol))), float(np.float32(trans_tol)) ** 2


def test_k130_is_past_one_trip_of_both_loops():
    f = CR.k130()
    P = len(f.pairs)
    assert f.n_sets == 130 and P == 8385 and P > 2048 * 4 and P % 4 and len(f.bad) == CR.K130_BAD
    assert len({(min(a, b), max(a, b)) for a, b in f.pairs.tolist()}) == P and 3000 < (f.pairs[:, 0] > f.pairs[:, 1]).sum() < 5400
    degree = np.bincount(f.pairs.reshape(-1), minlength=130)
    assert (np.minimum(degree[f.pairs[:, 0]], degree[f.pairs[:, 1]]) == 129).all()  # every pair's shorter list: three trips of 64 lanes (64 + 64 + 1)
    late = np.arange(P) >= 8192  # the pairs of the second grid trip
    res, s = CR.cycles(130, f.pairs, f.rt, *_thr(f), min_ok=f.params["min_ok"], max_rounds=64, keep=f.keep)
    drops = np.bincount(res["dropped_round"], minlength=s["rounds"] + 1).tolist()
    print("k130", s, "drops by round", drops, "late pairs by round", np.bincount(res["dropped_round"][late]).tolist(), "late alive", res["alive"][late].sum())
    assert (s["rounds"], s["stable"], s["alive"], s["edges"], s["triangles"], s["consistent"]) == CR.K130_SUMMARY and s["rounds"] >= 4 and s["stable"] == 1
    assert 0 < s["alive"] < s["edges"] == P and drops == CR.K130_DROPS
    assert len(set(res["dropped_round"][late & (res["dropped_round"] > 0)].tolist())) >= 2 and res["alive"][late].any()
    assert (res["cycles"] == 128).all() and (res["alive"][f.keep != 0] == 1).all() and 0 < f.keep.sum() < P and f.keep[late].any() and not f.keep[late].all()
    # cut short: not stable
    res, s = CR.cycles(130, f.pairs, f.rt, *_thr(f), min_ok=f.params["min_ok"], max_rounds=CR.K130_SHORT, keep=f.keep)
    assert (s["rounds"], s["stable"]) == (CR.K130_SHORT, 0) and CR.K130_SHORT < CR.K130_SUMMARY[0] and s["alive"] == P - sum(drops[1:CR.K130_SHORT + 1])
    # without the keep bytes the whole list unravels
    res, s = CR.cycles(130, f.pairs, f.rt, *_thr(f), min_ok=f.params["min_ok"], max_rounds=64)
    print("k130, no keep", s, np.bincount(res["dropped_round"]).tolist())
    assert (s["rounds"], s["stable"], s["alive"]) == CR.K130_NO_KEEP
    # the repeats: runs of equal neighbours in lists longer than a wave
    g = CR.k130_repeats()
    assert len(g.pairs) == P + 200 and (g.pairs[P:P + 100, 0] == f.pairs[:, 1][_index_of(f, g.pairs[P:P + 100, ::-1])]).all()
    res, s = CR.cycles(130, g.pairs, g.rt, *_thr(g), min_ok=g.params["min_ok"], max_rounds=64, keep=g.keep)
    print("k130_repeats", s, np.bincount(res["dropped_round"]).tolist(), "cycles", res["cycles"].min(), res["cycles"].max())
    assert (s["rounds"], s["stable"], s["alive"], s["edges"], s["triangles"], s["consistent"]) == CR.K130_REPEATS_SUMMARY
    assert s["triangles"] > 357760 and res["cycles"].max() > 128 and 0 < s["alive"] < s["edges"] and s["stable"] == 1


def _index_of(f, pairs):
    where = {tuple(ab): p for p, ab in enumerate(f.pairs.tolist())}
    return np.array([where[tuple(ab)] for ab in np.asarray(pairs).tolist()])


def test_exact24_is_integers_and_sits_on_the_cuts():
    f = CR.exact24()
    assert f.n_sets == 24 and len(f.pairs) == 276 and len(f.bad) == 92 and len(CR.GROUP24) == 24
    assert all((g @ g.T == np.eye(3)).all() for g in CR.GROUP24) and len({g.tobytes() for g in CR.GROUP24}) == 24
    tp, tq, tr_, tr, e2 = CR.exact24_integers()
    assert len(tp) == 2024 and sorted(zip(tp.tolist(), tq.tolist(), tr_.tolist())) == sorted(zip(*(x.tolist() for x in CR.triangles(f.pairs, np.ones(276, bool)))))
    ftr, fe2 = CR.errors(f.pairs, f.rt, tp, tq, tr_)
    assert (ftr == tr).all() and (fe2 == e2).all()  # exactly: every value is a small integer
    print("exact24 tr", dict(zip(*(x.tolist() for x in np.unique(tr, return_counts=True)))), "e2 <= 4", [int((e2 == v).sum()) for v in range(5)], "max", e2.max())
    assert set(tr.tolist()) == {3, 1, 0, -1} and e2.min() == 0
    counts = {}
    for (rot_tol, trans_tol), planted in CR.EXACT24_CUTS.items():
        tr_min, e2_max = _cut(rot_tol, trans_tol)
        good = (tr >= tr_min) & (e2 <= e2_max)
        res, s = CR.cycles(24, f.pairs, f.rt, tr_min, e2_max, min_ok=3)
        print("exact24", rot_tol, trans_tol, "tr_min", tr_min, "e2_max", e2_max, "consistent", good.sum(), s)
        assert ((ftr >= tr_min) & (fe2 <= e2_max)).tolist() == good.tolist() and s["consistent"] == good.sum() == planted
        ok = sum(np.bincount(role[good], minlength=276) for role in (tp, tq, tr_))
        assert (res["ok"] == ok).all()
        counts[(rot_tol, trans_tol)] = int(good.sum())
    # the cuts are inclusive and there are triangles on them
    assert _cut(0.0, 0.0) == (3.0, 0.0) and _cut(0.0, 1.0)[1] == 1.0 and _cut(0.0, 2.0)[1] == 4.0
    assert ((tr == 3) & (e2 == 0)).sum() == counts[(0.0, 0.0)] > 0  # tr == tr_min and e2 == e2_max at once: > or < would leave nothing
    assert ((tr == 3) & (e2 == 1)).sum() == counts[(0.0, 1.0)] - counts[(0.0, 0.0)] > 0
    assert ((tr == 3) & (e2 == 4)).sum() > 0 and ((tr == 3) & (e2 <= 4)).sum() == counts[(0.0, 2.0)] > counts[(0.0, 1.0)] + ((tr == 3) & (e2 == 4)).sum()
    # a loop off by exactly a half turn is not consistent even at the largest rot_tol: tr_min = -1 + 7.6e-15
    assert -1.0 < _cut(CR.PI32, 1.0)[0] < -1.0 + 1e-14 and ((tr == -1) & (e2 <= 1)).sum() > 0
    assert counts[(CR.PI32, 1.0)] == ((tr > -1) & (e2 <= 1)).sum()
    quarter, third = float(np.float32(np.pi / 2)), float(np.float32(2 * np.pi / 3))
    assert counts[(quarter, 1.0)] == ((tr >= 1) & (e2 <= 1)).sum() and counts[(third, 0.0)] == ((tr >= 0) & (e2 == 0)).sum()


def test_scaling_the_translations_scales_max_e2_alone():
    for f, min_ok, keep in ((CR.k24(), 3, None), (CR.k130(), CR.K130_MIN_OK, CR.k130().keep)):
        base, bs = CR.cycles(f.n_sets, f.pairs, f.rt, *_thr(f), min_ok=min_ok, max_rounds=64, keep=keep)
        for k in (-100, -40, 40, 100):
            g = CR.scaled(f, k)
            assert (g.rt[:, :9] == f.rt[:, :9]).all() and (g.rt[:, 9:].astype(np.float64) == np.ldexp(f.rt[:, 9:].astype(np.float64), k)).all()
            assert _thr(g)[1] == math.ldexp(_thr(f)[1], 2 * k)
            res, s = CR.cycles(g.n_sets, g.pairs, g.rt, *_thr(g), min_ok=min_ok, max_rounds=64, keep=keep)
            assert s.tobytes() == bs.tobytes()
            for name in res.dtype.names:
                want = np.ldexp(base["max_e2"], 2 * k) if name == "max_e2" else base[name]
                assert res[name].tobytes() == want.tobytes(), (k, name)
        g = CR.scaled(f, -140)  # subnormal floats: valid input, no covariance claimed
        assert np.isfinite(g.rt).all() and 0 < g.params["trans_tol"] < np.finfo(np.float32).tiny
        assert ((g.rt[:, 9:] != 0) & (np.abs(g.rt[:, 9:]) < np.finfo(np.float32).tiny)).any()
        g = CR.scaled(f, 120)
        assert np.isfinite(g.rt).all() and np.isfinite(np.float32(g.params["trans_tol"]))


def test_hostile24_is_finite_and_overflows_only_e2():
    f = CR.hostile24()
    assert np.isfinite(f.rt).all() and (f.pairs == CR.k24().pairs).all()
    exponent = (f.rt.view(np.uint32) >> 23) & 0xFF
    assert exponent.min() == 0 and exponent.max() == 254 and len(set(exponent.reshape(-1).tolist())) > 250 and (f.rt < 0).any() and (f.rt > 0).any()
    assert (f.rt.view(np.uint32) == 0x80000000).any() and (f.rt == 0).all(axis=1).any()  # -0.0; one all-zero record
    assert ((exponent == 0) & (f.rt != 0)).any()  # subnormals
    assert (f.rt[f.bad] == CR.FLT_MAX).all() and len(f.bad) == 3
    for min_ok in (0, 1):
        res, s = CR.cycles(24, f.pairs, f.rt, *_thr(f), min_ok=min_ok)
        print("hostile24", min_ok, s, "max_e2 inf", np.isinf(res["max_e2"]).sum(), "min_trace", res["min_trace"].min(), res["min_trace"].max())
        assert (res["status"] == SC_OK).all() and s["edges"] == 276 and s["triangles"] == 2024
        assert not np.isnan(res["min_trace"]).any() and not np.isnan(res["max_e2"]).any() and np.isfinite(res["min_trace"]).all()
        assert (res["max_e2"][f.bad] == np.inf).all() and np.isinf(res["max_e2"]).sum() == 3 and (res["max_e2"] >= 0).all()
        assert (res["min_trace"] < -1e100).any() and (res["min_trace"] < -1.0).sum() > 200
        assert s["alive"] == (276 if min_ok == 0 else 276 - (res["ok"] == 0).sum())
    for directions in range(8):
        g = CR.flt_max_triangle(directions)
        res, s = CR.cycles(3, g.pairs, g.rt, *_thr(g))
        inverted = bin(directions ^ 4).count("1")  # pairs 0 and 1 are inverted where stored reversed, pair 2 (c -> a) where it is not
        print("FLT_MAX triangle", g.pairs.tolist(), res["min_trace"][0], res["max_e2"][0])
        assert (s["triangles"], s["consistent"], s["alive"]) == (1, 0, 0) and np.isfinite(res["min_trace"]).all() and abs(res["min_trace"][0]) > 1e116
        assert (res["max_e2"] == res["max_e2"][0]).all() and np.isinf(res["max_e2"][0]) == bool(directions & 1) and not np.isnan(res["max_e2"]).any()
    assert CR.cycles(3, [(1, 0), (2, 1), (0, 2)], g.rt, *_thr(g))[0]["max_e2"].view(np.uint64).tolist() == [0x7FF0000000000000] * 3
    assert CR.cycles(3, [(0, 1), (1, 2), (0, 2)], g.rt, *_thr(g))[0]["max_e2"].max() < 3.78e233
