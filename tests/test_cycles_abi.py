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
