"""CPU suite: the surface of sc_pairs_sync (include/saccot.h) — the four exports, the Python mirror, the layouts of sc_sync_params,
sc_sync_set, sc_sync_pair and sc_sync_summary compiled in C99, the default parameters, sc_sync_thresholds, every rule that refuses a
call with its text (the host-only rules run under the sanitizers, in a program of their own) — and the Python restatement
(tests/sync_ref.py) that the GPU tests compare against: its input families are checked for what they are used for.  No compute call
reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import cycles_ref as CR
import sync_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_sync_default_params", "sc_sync_thresholds", "sc_pairs_sync", "sc_pairs_sync_device")
SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def _section():
    header = _header()
    return header[header.index("sc_pairs_sync ---"):header.index("two-phase form for one-process-per-GPU sharding")]


def test_sync_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    for method in ("pairs_sync", "pairs_sync_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert callable(pkg.make_sync_params) and callable(pkg.sync_thresholds)
    for struct, dtype, ref in (("ScSyncSet", "SYNC_SET_DTYPE", SR.SET_DTYPE), ("ScSyncPair", "SYNC_PAIR_DTYPE", SR.PAIR_DTYPE),
                               ("ScSyncSummary", "SYNC_SUMMARY_DTYPE", SR.SUMMARY_DTYPE)):
        S, D = getattr(pkg, struct), getattr(pkg, dtype)
        assert np.dtype(S) == D and D.itemsize == C.sizeof(S) == ref.itemsize and list(D.names) == list(ref.names)
        assert [D.fields[f][1] for f in D.names] == [ref.fields[f][1] for f in ref.names] == [getattr(S, f).offset for f in D.names]
        assert [D.fields[f][0] for f in D.names] == [ref.fields[f][0] for f in ref.names]
    assert (pkg.SC_SYNC_STATUS, SR.STATUS, SR.UNREACHED) == (1, 1, SC_ENOHYP)


def test_the_minor_version_stays_and_the_section_is_its_own(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_PAIRS_SYNC 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10
    # not inside the span that tests/test_cycles_abi.py slices
    cycles = header[header.index("sc_pairs_cycles ---"):header.index("sc_match_guided_poses ---")]
    assert "sc_pairs_sync" not in cycles and "sc_sync_" not in cycles
    assert header.index("sc_pairs_sync ---") > header.index("sc_match_guided_poses ---")


def test_the_section_states_the_limits_and_every_rule():
    flat = " ".join(_section().replace("\n * ", "\n").split())
    for word in ("Not here / not built:", "conjugate gradients on the graph Laplacian", "Gauss-Newton on the pairs' 6 x 6 information matrices",
                 "it DIFFUSES", "is a STOPPING RULE, not an accuracy bound", "a bare ring of 40 sets needs 89 rounds", "SC_ENOHYP"):
        assert word in flat, word
    for rule in ("r2_max = 2.0 * (double)rot_tol * (double)rot_tol", "e2_max = (double)trans_tol * (double)trans_tol",
                 "1 + 2 cos(rot_tol) is exactly 3.0 below 2e-8", "X_a = X_b o T", "P = X_{k-1}(n) o T_p(s->n)", "Entry i adds into slot i mod 64, in increasing i",
                 "acc[c] = acc[c] + w_p * P[c]", "accW = accW + w_p", "for h = 32, 16, 8, 4, 2, 1: slot[j] = slot[j] + slot[j + h] for j < h",
                 "R' = rot(M), t'_i = c_i / W", "dot(a, b) = (a_0 * b_0 + a_1 * b_1) + a_2 * b_2", "zeta = (beta - alpha) / (gamma + gamma)",
                 "tt = 1.0 / (|zeta| + sqrt(zeta * zeta + 1.0))", "cs = 1.0 / sqrt(tt * tt + 1.0), sn = cs * tt",
                 "B_p[r] = cs * x - sn * y, B_q[r] = sn * x + cs * y", "(a x b)_0 = a_1 * b_2 - a_2 * b_1",
                 "R'_rc = (v1[r] * u1[c] + v2[r] * u2[c]) + v3[r] * u3[c]", "dR2 > r2_max, or dt2 > e2_max: both cuts inclusive on the quiet side",
                 "Q = X_K(b) o T_p(a->b)", "a copy, a memset, max_rounds + 2 launches"):
        assert rule in flat, rule
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "2f-2" in integration and "sc_pairs_sync_device" in integration
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.9d" in design and "sync_round_kernel" in design


def test_the_struct_layouts_and_the_macros_in_c(pkg, tmp_path):
    exe = str(tmp_path / "sync_layout")
    P, S, R, M = "sc_sync_params", "sc_sync_set", "sc_sync_pair", "sc_sync_summary"
    pf = ("size", "anchor", "max_rounds", "flags", "rot_tol", "trans_tol", "reserved")
    sf = ("Rt", "status", "known_round", "used", "degenerate", "X")
    rf = ("status", "used", "r2", "e2", "reserved")
    mf = ("rounds", "converged", "known", "used", "changed_last", "reserved")
    fields = []
    for name, fs in ((P, pf), (S, sf), (R, rf), (M, mf)):
        fields += [f"sizeof({name})"] + [f"offsetof({name}, {f})" for f in fs]
    consts = ["SC_SYNC_STATUS", "SC_HAS_PAIRS_SYNC"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("' + "%zu " * len(fields) + "%u " * len(consts)
           + '", ' + ", ".join(fields) + ", " + ", ".join(f"(unsigned){c}" for c in consts) + ");return 0;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[:8] == [32, 0, 4, 8, 12, 16, 20, 24] == [C.sizeof(pkg.ScSyncParams)] + [getattr(pkg.ScSyncParams, f).offset for f in pf]
    assert got[8:15] == [160, 0, 48, 52, 56, 60, 64] == [C.sizeof(pkg.ScSyncSet)] + [getattr(pkg.ScSyncSet, f).offset for f in sf]
    assert got[15:21] == [32, 0, 4, 8, 16, 24] == [C.sizeof(pkg.ScSyncPair)] + [getattr(pkg.ScSyncPair, f).offset for f in rf]
    assert got[21:28] == [32, 0, 4, 8, 12, 16, 20] == [C.sizeof(pkg.ScSyncSummary)] + [getattr(pkg.ScSyncSummary, f).offset for f in mf]
    assert got[28:] == [1, 1]


def test_default_params_and_null_arguments(pkg):
    L = pkg.load_library()
    sp = pkg.ScSyncParams()
    sp.reserved[1] = 9; sp.rot_tol = 0.5; sp.flags = 1; sp.anchor = 7
    assert L.sc_sync_default_params(C.byref(sp)) == SC_OK
    assert (sp.size, sp.anchor, sp.max_rounds, sp.flags, sp.rot_tol, sp.trans_tol, list(sp.reserved)) == (32, 0, 32, 0, 0.0, 0.0, [0, 0])
    assert L.sc_sync_default_params(None) == SC_EINVAL
    assert bytes(pkg.make_sync_params()) == bytes(sp)  # the Python defaults are the library's
    mk = pkg.make_sync_params(0.25, 0.5, anchor=3, max_rounds=7, flags=1)
    assert (mk.size, mk.anchor, mk.max_rounds, mk.flags, mk.rot_tol, mk.trans_tol) == (32, 3, 7, 1, 0.25, 0.5)
    # (a context cannot exist here — sc_create fails without a GPU — so the NULL context is what is tried; the GPU suite tries the
    # rest with a context and reads sc_last_error, and the program below checks every rule's text)
    pairs = (C.c_uint32 * 2)(0, 1)
    assert L.sc_pairs_sync(None, 2, pairs, 1, C.byref(mk), None, 48, None, 4, None, None, None, None) == SC_EINVAL
    assert L.sc_pairs_sync_device(None, 2, pairs, 1, C.byref(mk), None, 48, None, 4, None, None, None, None) == SC_EINVAL


def test_the_thresholds(pkg):
    L = pkg.load_library()
    out = (C.c_double * 2)()
    for rot, trans in ((0.0, 0.0), (1e-4, 1e-4), (0.25, 0.5), (1.0, 3.0), (3.1415927, 1e19), (1e-8, 1e-20), (2.0 ** -4, 2.0 ** -4)):
        sp = pkg.make_sync_params(rot, trans)
        assert L.sc_sync_thresholds(C.byref(sp), out) == SC_OK
        rot32, trans32 = float(np.float32(rot)), float(np.float32(trans))
        assert out[0] == 2.0 * rot32 * rot32 and out[1] == trans32 * trans32  # exactly: two products each
        assert pkg.sync_thresholds(sp) == (out[0], out[1]) == SR.thresholds(rot, trans)
    assert out[0] == 2.0 ** -7 and out[1] == 2.0 ** -8
    sp = pkg.make_sync_params(1e-8, 0.0)
    assert pkg.sync_thresholds(sp)[0] > 0.0 and 1.0 + 2.0 * np.cos(np.float64(np.float32(1e-8))) == 3.0  # a trace's threshold would be no threshold
    assert L.sc_sync_thresholds(None, out) == SC_EINVAL and L.sc_sync_thresholds(C.byref(sp), None) == SC_EINVAL
    for bad in (pkg.make_sync_params(-0.1, 0.0), pkg.make_sync_params(3.2, 0.0), pkg.make_sync_params(0.1, -1.0), pkg.make_sync_params(float("nan"), 0.0),
                pkg.make_sync_params(0.1, float("inf")), pkg.make_sync_params(0.1, 0.1, max_rounds=257), pkg.make_sync_params(0.1, 0.1, max_rounds=0),
                pkg.make_sync_params(0.1, 0.1, flags=2)):
        assert L.sc_sync_thresholds(C.byref(bad), out) == SC_EINVAL
    wrong = pkg.make_sync_params(0.1, 0.1); wrong.size = 28
    assert L.sc_sync_thresholds(C.byref(wrong), out) == SC_EINVAL


def test_the_host_rules_under_the_sanitizers(tmp_path):
    """Every refusal rule of sc_sync_check.hpp with its text, the thresholds, the bytes read of a strided use array, the workspace
    offsets and the staged image of a list: tests/native/sync_check_main.cpp, a program of its own built with
    -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "sync_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "sync_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


# ---- the reference itself: the families are what they are used for ----------------------------------------------------------------
def _run(f, **kw):
    p = dict(f.params); p.update(kw)
    thr = SR.thresholds(p.pop("rot_tol"), p.pop("trans_tol"))
    statuses = f.statuses if p.pop("flags", 0) & SR.STATUS else None
    return SR.sync(f.n_sets, f.pairs, f.rt, *thr, use=f.use, weight=f.weight, statuses=statuses, **p)


def _noise_put_in(noisy, exact):
    """the largest Frobenius distance of a noisy record's rotation from the exact one's, and the largest distance of the translations"""
    d = noisy.rt.astype(np.float64) - exact.rt.astype(np.float64)
    return float(np.sqrt((d[:, :9] ** 2).sum(axis=1)).max()), float(np.sqrt((d[:, 9:] ** 2).sum(axis=1)).max())


def test_the_noisy_families_converge_to_the_ground_truth():
    """The bound on a set's error is the noise put into the records plus the floor — what the reference leaves of the same list with
    exact (un-noised, fp32-rounded) records.  Measured (rotation: Frobenius distance; translation: length units):
      k24    noise put in 7.4e-3, 1.1e-2   floor 7.2e-9, 2.9e-8   error 2.3e-3, 1.6e-3   rounds 4 (exact: 2)
      g512   noise put in 7.4e-3, 1.3e-2   floor 1.5e-8, 3.6e-8   error 3.4e-3, 3.7e-3   rounds 8 (exact: 4)
    (the translation noise is what the records differ by: the turn of up to 0.3 degrees moves a record's t as well as the shift of up
    to 3e-3 does)."""
    for name, family, rounds in (("k24", SR.k24, (4, 5)), ("g512", SR.g512, (7, 9))):
        f, exact = family(True), family(False)
        assert (f.pairs == exact.pairs).all()
        noise = _noise_put_in(f, exact)
        sets0, _pairs0, s0 = _run(exact)
        floor = SR.errors(sets0, exact)
        sets, pairs, s = _run(f)
        err = SR.errors(sets, f)
        print(name, "noise put in", noise, "floor", floor, "error", err, "summary", s, "exact summary", s0)
        assert 0.9 * np.sqrt(2) * np.deg2rad(SR.NOISE_DEG) < noise[0] <= np.sqrt(2) * np.deg2rad(SR.NOISE_DEG) * 1.0001 and noise[1] > 0.9 * SR.NOISE_TRANS
        assert s0["converged"] == 1 and s["converged"] == 1 and rounds[0] <= s["rounds"] <= rounds[1] and s["known"] == f.n_sets and s["used"] == len(f.pairs)
        assert floor[0] < 1e-7 and floor[1] < 1e-6
        assert err[0] <= noise[0] + floor[0] and err[1] <= noise[1] + floor[1]
        assert (sets["status"] == SC_OK).all() and (sets["degenerate"] == 0).all() and (pairs["used"] == 1).all() and (pairs["r2"] > 0).all()
        assert (sets["Rt"] == sets["X"].astype(np.float32)).all() and sets["known_round"].max() == (1 if name == "k24" else 3)
        # the residuals are the records' noise, not more: r2 is a squared Frobenius distance
        assert pairs["r2"].max() < (2 * noise[0]) ** 2 and pairs["e2"].max() < (2 * noise[1]) ** 2


def test_a_bare_chain_is_reached_a_set_a_round():
    f = SR.chain()
    assert f.n_sets == 42 and len(f.pairs) == 41 and (f.pairs[:, 0] > f.pairs[:, 1]).sum() == 21
    sets, pairs, s = _run(f, max_rounds=64)
    assert sets["known_round"].tolist() == list(range(42)) and (sets["status"] == SC_OK).all()
    assert (s["rounds"], s["converged"], s["known"], s["used"], s["changed_last"]) == (42, 1, 42, 41, 0)
    assert sets["used"].tolist() == [0] + [2] * 40 + [1]
    sets, pairs, s = _run(f, max_rounds=42)
    assert (s["rounds"], s["converged"]) == (42, 1)
    sets, pairs, s = _run(f, max_rounds=41)
    assert (s["rounds"], s["converged"], s["known"], s["changed_last"]) == (41, 0, 42, 1)
    sets, pairs, s = _run(f, max_rounds=20)
    assert (s["rounds"], s["converged"], s["known"], s["used"], s["changed_last"]) == (20, 0, 21, 20, 1)
    assert (sets["status"][:21] == SC_OK).all() and (sets["status"][21:] == SC_ENOHYP).all() and not sets["X"][21:].any() and not sets["Rt"][21:].any()
    assert not sets["known_round"][21:].any() and sets["known_round"][:21].tolist() == list(range(21))
    assert pairs["used"].tolist() == [1] * 20 + [0] * 21 and not pairs["r2"][20:].any() and not pairs["e2"][20:].any()
    err = SR.errors(sets[:21], SR.Family(21, f.pairs[:20], f.rt[:20], f.R[:21], f.t[:21]))
    assert err[0] < 1e-6 and err[1] < 1e-5  # exact records: what is reached is right


def test_a_second_component_is_never_reached():
    f = SR.two_components()
    sets, pairs, s = _run(f)
    assert (s["known"], s["used"], s["converged"]) == (24, 276, 1) and (sets["status"][24:] == SC_ENOHYP).all() and not sets["X"][24:].any()
    assert (pairs["used"][276:] == 0).all() and (pairs["status"] == SC_OK).all() and (sets["used"][24:] == 0).all()
    alone = _run(SR.k24())
    assert sets[:24].tobytes() == alone[0].tobytes() and pairs[:276].tobytes() == alone[1].tobytes()
    # anchored in the second world it is the first that is not reached
    sets, pairs, s = _run(f, anchor=26)
    assert s["known"] == 6 and (sets["status"][:24] == SC_ENOHYP).all() and (sets["status"][24:] == SC_OK).all() and s["used"] == 15
    assert sets["X"][26].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and sets["known_round"][26] == 0


def test_permuting_the_list_leaves_every_set_bit_identical():
    """(lists without repeated pairs: among entries to one neighbour it is the pair's index that orders a set's sorted list)"""
    for f in (SR.k24(), SR.g512(), SR.chain()):
        assert len({(min(a, b), max(a, b)) for a, b in f.pairs.tolist()}) == len(f.pairs)
        base = _run(f, max_rounds=64)
        perm = np.random.default_rng(5).permutation(len(f.pairs))
        got = SR.sync(f.n_sets, f.pairs[perm], f.rt[perm], *SR.thresholds(SR.TOL, SR.TOL), max_rounds=64)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1][perm].tobytes() and got[2].tobytes() == base[2].tobytes()


def test_two_opposed_predictions_are_degenerate():
    f = SR.degenerate()
    sets, pairs, s = _run(f)
    assert sets["degenerate"].tolist() == [0, 1, 0, 0] and sets["status"].tolist() == [SC_OK, SC_ENOHYP, SC_OK, SC_OK]
    assert sets["used"].tolist() == [0, 2, 1, 1] and sets["known_round"].tolist() == [0, 0, 1, 1] and not sets["X"][1].any()
    assert (s["rounds"], s["converged"], s["known"], s["used"]) == (2, 1, 3, 2) and pairs["used"].tolist() == [1, 1, 0, 0]
    M = [np.array([x]) for x in (2.0, 0, 0, 0, 0, 0, 0, 0, 0)]  # I + diag(1, -1, -1)
    assert not np.isfinite(np.array(SR.rot(M))).all()
    # with max_rounds 5 the sum is met in rounds 2 .. K only while a set changes: K is 2, so once
    assert _run(f, max_rounds=5)[0]["degenerate"].tolist() == [0, 1, 0, 0]


def test_rot_is_the_nearest_rotation():
    rng = np.random.default_rng(9)
    Ms = rng.normal(size=(200, 9))
    Ms[:50] = [(CR.rotation(rng.normal(size=3), rng.uniform(0, np.pi)) * rng.uniform(0.5, 30) + rng.normal(size=(3, 3)) * 0.01).ravel() for _ in range(50)]
    R = np.stack(SR.rot([Ms[:, c].copy() for c in range(9)]), axis=1).reshape(-1, 3, 3)
    for M, got in zip(Ms.reshape(-1, 3, 3), R):
        U, _s, Vt = np.linalg.svd(M)
        want = U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt
        assert np.abs(got @ got.T - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(got) - 1) < 1e-13
        if _s[1] > 1e-3 * _s[0]:  # (two well-separated directions: the construction's domain)
            assert np.abs(got - want).max() < 1e-9, (M, got, want)


def test_the_cut_family_sits_on_the_cut():
    f = SR.cut24()
    exact = CR.exact24()
    clean = np.ones(276, bool); clean[exact.bad] = False
    touched = np.flatnonzero((f.pairs == SR.CUT_SET).any(axis=1) & (f.pairs == 0).any(axis=1))
    assert (f.pairs == exact.pairs).all() and len(touched) == 1
    same = clean.copy(); same[touched] = False
    assert (f.rt[same] == exact.rt[same].astype(np.float32)).all()  # exact24's world where exact24 left it alone
    tp, tq, tr_, tr, e2 = CR.exact24_integers()
    whole = clean[tp] & clean[tq] & clean[tr_]
    assert whole.sum() > 100 and (tr[whole] == 3).all() and (e2[whole] == 0).all()  # that world closes every loop exactly
    assert (f.rt == np.round(f.rt * 8) / 8).all() and f.use.sum() == 276 - 21 and SR.thresholds(0.0, SR.CUT_TOL) == (0.0, 2.0 ** -8)
    below = float(np.nextafter(np.float32(SR.CUT_TOL), np.float32(0)))
    trace, trace_below = [], []
    on = SR.sync(24, f.pairs, f.rt, *SR.thresholds(0.0, SR.CUT_TOL), use=f.use, trace=trace)
    under = SR.sync(24, f.pairs, f.rt, *SR.thresholds(0.0, below), use=f.use, trace=trace_below)
    # round 2 moves the set by exactly 2^-4: dt2 is e2_max to the bit, dR2 is 0 = r2_max, and the set counts as quiet
    changed, dR2, dt2, update = trace[1]
    assert update[SR.CUT_SET] and dt2[SR.CUT_SET] == 2.0 ** -8 == SR.thresholds(0.0, SR.CUT_TOL)[1] and dR2[SR.CUT_SET] == 0.0 and not changed.any()
    assert (on[2]["rounds"], on[2]["converged"], on[2]["known"]) == (2, 1, 24) and len(trace) == 2
    # one ulp lower it is changed, and a third round runs
    changed, dR2, dt2, update = trace_below[1]
    assert dt2[SR.CUT_SET] == 2.0 ** -8 > SR.thresholds(0.0, below)[1] and changed.tolist() == [s == SR.CUT_SET for s in range(24)]
    assert (under[2]["rounds"], under[2]["converged"]) == (3, 1) and len(trace_below) == 3
    assert on[0]["X"][SR.CUT_SET].tobytes() != under[0]["X"][SR.CUT_SET].tobytes()
    # every other set is exact in round 1 and the rotations stay exact throughout
    want = SR.truth(f)
    assert (on[0]["X"][:, :9] == want[:, :9]).all() and (under[0]["X"][:, :9] == want[:, :9]).all()


def test_invalid_unused_and_unweighted_pairs_take_part_in_nothing():
    f = SR.k24()
    P = len(f.pairs)
    rt = f.rt.copy(); rt[5, 3] = np.nan; rt[6, 10] = np.inf
    st = np.zeros(P, np.int32); st[9] = SC_ENOHYP
    pairs = f.pairs.copy(); pairs[11] = (7, 7)
    use = np.ones(P, np.uint32); use[12] = 0; use[13] = 0x80000000
    w = np.ones(P, np.float32); w[14] = 0; w[15] = -1; w[16] = np.inf; w[17] = np.nan; w[18] = 2.5; w[19] = 1e-3
    out = [5, 6, 9, 11, 12, 14, 15, 16, 17]
    sets, res, s = SR.sync(24, pairs, rt, *SR.thresholds(SR.TOL, SR.TOL), use=use, weight=w, statuses=st)
    assert res["status"][[5, 6, 9, 11]].tolist() == [SC_EINVAL, SC_EINVAL, SC_ENOHYP, SC_OK] and not res["used"][out].any() and res["used"].sum() == P - len(out)
    assert not res["r2"][out].any() and not res["e2"][out].any() and s["used"] == P - len(out) and s["known"] == 24
    others = np.setdiff1d(np.arange(P), out)
    alone = SR.sync(24, pairs[others], rt[others], *SR.thresholds(SR.TOL, SR.TOL), weight=w[others])
    # (not bit for bit: an entry that is not live keeps its index, so the slots of the two lists hold different entries)
    assert np.abs(alone[0]["X"] - sets["X"]).max() < 1e-13 and (alone[0]["used"] == sets["used"]).all() and alone[2]["rounds"] == s["rounds"]
    assert np.abs(alone[1]["r2"] - res["r2"][others]).max() < 1e-15 and (alone[1]["used"] == 1).all()
    # the weights matter: the same list with every weight 1 is another result
    plain = SR.sync(24, pairs[others], rt[others], *SR.thresholds(SR.TOL, SR.TOL))
    assert plain[0]["X"].tobytes() != sets["X"].tobytes()


# ---- the families of tests/test_gpu_pairs_sync_range.py: what the reference measures on them, as literals -------------------------
def _summary(s, n=4):
    return tuple(int(s[name]) for name in ("rounds", "converged", "known", "used", "changed_last")[:n])


RCUT_BELOW = float(np.nextafter(np.float32(SR.RCUT_TOL), np.float32(0)))
RCUT_ROUNDS = {SR.RCUT_TOL: (2, 1), RCUT_BELOW: (3, 1)}  # rot_tol -> (rounds, converged)
RCUT_DEGENERATE, RCUT_USED, RCUT_R1 = [0, 0, 1, 1], [0, 3, 2, 2], [1, 0, 0, 0, -1, 0, 0, 0, -1]
EXACT24_SUMMARY, EXACT_RING_SUMMARY = (2, 1, 24, 276), (13, 1, 24, 24)
EXACT_RING_HOPS = list(range(13)) + list(range(11, 0, -1))
K24_SUMMARY = (4, 1, 24, 276)  # at every exact scale
SCALE_UNDER_SUMMARY = (32, 0, 24, 276, 23)
WEIGHT_SCALED_SUMMARY = (26, 1, 24, 276)  # at k = 0, -100 and 100
WEIGHT_UNDER = ((28, 1, 24, 228), 48, 166)  # at k = -140: the summary, the weights that are 0.0, those that are subnormal
WEIGHTS_RANGE_SUMMARY = (32, 0, 24, 274, 23)
# hostile: (anchor, max_rounds) -> summary; the sets whose degenerate is 1; the components of Rt that are not finite
HOSTILE = {(0, 32): ((32, 0, 24, 276, 23), [3, 7], 69), (0, 256): ((256, 0, 24, 276, 23), [3, 7], 69), (11, 32): ((32, 0, 24, 276, 23), [], 69)}
RING40 = {(1e-6, 256): (256, 0, 40, 40, 18), (1e-4, 256): (120, 1, 40, 40, 0), (1e-4, 1): (1, 0, 3, 2, 2)}  # (tolerances, max_rounds) -> summary
SPARSE_SUMMARY = (42, 1, 42, 41, 0)
# family -> the anchor, the second call's summary (hostile: the anchor aside every set's Rt has an infinite component, under SC_OK)
SELF_STAR = {"k24": (3, (2, 1, 24, 23)), "two_components": (0, (2, 1, 24, 23)), "hostile": (0, (1, 1, 1, 0))}


def _rounds_with(compare, trace, r2_max, e2_max):
    """(rounds, converged) of a run whose rounds are `trace`, the header's rule for `changed` restated with `compare` for its `>`"""
    known = None
    for k, (_changed, dR2, dt2, update) in enumerate(trace, 1):
        fresh = update if known is None else update & ~known
        if not (update & (fresh | compare(dR2, r2_max) | compare(dt2, e2_max))).any():
            return k, 1
        known = update if known is None else known | update
    return len(trace), 0


def test_rcut_sits_on_the_rotation_cut_and_a_known_set_meets_a_degenerate_sum():
    f = SR.rcut()
    assert f.n_sets == 4 and f.pairs.tolist() == [[1, 0], [2, 0], [3, 0], [1, 2], [1, 3]] and not f.rt[:, 9:].any()
    assert SR.thresholds(SR.RCUT_TOL, 0.0) == (8.0, 0.0) and SR.thresholds(RCUT_BELOW, 0.0)[0] < 8.0
    traces = {}
    for tol, want in RCUT_ROUNDS.items():
        traces[tol] = []
        sets, pairs, s = _run(f, rot_tol=tol, trace=traces[tol])
        assert _summary(s, 2) == want and len(traces[tol]) == want[0], tol
        assert sets["degenerate"].tolist() == RCUT_DEGENERATE and sets["used"].tolist() == RCUT_USED and sets["X"][1][:9].tolist() == RCUT_R1
        assert (sets["status"] == SC_OK).all() and sets["known_round"].tolist() == [0, 1, 1, 1]  # sets 2 and 3 stay known, at the identity
        assert sets["X"][2].tolist() == sets["X"][3].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    # round 1: every set placed by the anchor alone; round 2: set 1 turns by exactly dR2 = 8.0 = r2_max and is quiet, sets 2 and 3
    # meet a sum of rank one and are not updated
    changed, dR2, dt2, update = traces[SR.RCUT_TOL][0]
    assert changed.tolist() == update.tolist() == [False, True, True, True]
    changed, dR2, dt2, update = traces[SR.RCUT_TOL][1]
    assert dR2[1] == 8.0 == SR.thresholds(SR.RCUT_TOL, 0.0)[0] and dt2[1] == 0.0 and update.tolist() == [False, True, False, False] and not changed.any()
    assert traces[RCUT_BELOW][1][0].tolist() == [False, True, False, False] and not traces[RCUT_BELOW][2][0].any()
    # the bite: the rule restated over the three rounds (a round's sums do not depend on the tolerances) agrees with the reference
    # with `>` at both tolerances, and with `>=` it runs a third round ON the cut
    full = traces[RCUT_BELOW]
    for tol, want in RCUT_ROUNDS.items():
        assert _rounds_with(np.greater, full, *SR.thresholds(tol, 0.0)) == want
    mutant = _rounds_with(np.greater_equal, full, *SR.thresholds(SR.RCUT_TOL, 1.0))  # (trans_tol 1: only the rotation cut is sat on)
    assert mutant == (3, 1) != RCUT_ROUNDS[SR.RCUT_TOL] and _rounds_with(np.greater, full, *SR.thresholds(SR.RCUT_TOL, 1.0)) == (2, 1)


def test_exact24_and_the_exact_ring_equal_the_integers():
    """the expectation is SR.integers: np.int64 products of the absolute poses, none of the reference's arithmetic"""
    cut = SR.cut24()
    for anchor in (0, 13):
        f = SR.exact24(anchor)
        assert (f.pairs == cut.pairs).all() and all((a == b).all() for a, b in zip(f.R, cut.R)) and (f.t == cut.t).all()  # cut24's world
        assert (f.rt == np.round(f.rt)).all() and f.t.dtype == np.int64 and np.abs(f.t).max() <= 8 and f.params["anchor"] == anchor
        want = SR.integers(f, anchor)
        assert want.dtype == np.int64 and want[anchor].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and (want == SR.truth(f, anchor)).all()
        sets, pairs, s = _run(f)
        assert _summary(s) == EXACT24_SUMMARY and (sets["X"] == want).all() and (sets["Rt"] == want).all()
        assert not pairs["r2"].any() and not pairs["e2"].any() and (pairs["used"] == 1).all()  # exactly 0.0, on all 276 pairs
    ring = SR.exact_ring()
    assert len(ring.pairs) == 24 and (ring.pairs[:, 0] > ring.pairs[:, 1]).sum() == 12 + 1 and (ring.t == cut.t).all()
    assert sorted(tuple(sorted(p)) for p in ring.pairs.tolist()) == sorted(tuple(sorted((i, (i + 1) % 24))) for i in range(24))
    sets, pairs, s = _run(ring)
    want = SR.integers(ring)
    assert _summary(s) == EXACT_RING_SUMMARY and (sets["X"] == want).all() and (sets["Rt"] == want).all() and not pairs["r2"].any() and not pairs["e2"].any()
    assert sets["known_round"].tolist() == EXACT_RING_HOPS == [min(i, 24 - i) for i in range(24)]


def test_scaled_translations_and_weights_are_exact_where_they_are_used_as_exact():
    base = SR.k24()
    sets0, pairs0, s0 = _run(base)
    assert _summary(s0) == K24_SUMMARY
    for k in SR.SCALES_EXACT:
        g = SR.scaled(k)
        assert (np.ldexp(g.rt[:, 9:].astype(np.float64), -k) == base.rt[:, 9:]).all() and (g.rt[:, :9] == base.rt[:, :9]).all()  # nothing was rounded
        assert np.ldexp(np.float64(np.float32(g.params["trans_tol"])), -k) == np.float32(SR.TOL) and np.isfinite(g.rt).all()
        sets, pairs, s = _run(g)
        assert s.tobytes() == s0.tobytes() and sets["X"][:, :9].tobytes() == sets0["X"][:, :9].tobytes() and pairs["r2"].tobytes() == pairs0["r2"].tobytes()
        assert sets["X"][:, 9:].tobytes() == np.ldexp(sets0["X"][:, 9:], k).tobytes() and pairs["e2"].tobytes() == np.ldexp(pairs0["e2"], 2 * k).tobytes()
        assert (pairs["e2"] > 0).all() and np.isfinite(pairs["e2"]).all()
    g = SR.scaled(SR.SCALE_UNDER)  # the tolerance underflows to 0.0 and translations are rounded to subnormals: no relation holds
    tiny = np.abs(g.rt[:, 9:])
    assert g.params["trans_tol"] == 0.0 and ((tiny > 0) & (tiny < np.finfo(np.float32).tiny)).sum() > 100
    assert (np.ldexp(g.rt[:, 9:].astype(np.float64), -SR.SCALE_UNDER) != base.rt[:, 9:]).any()
    assert _summary(_run(g)[2], 5) == SCALE_UNDER_SUMMARY
    w0 = SR.weight_scaled(0)
    e = np.frexp(w0.weight)[1] - 1
    assert e.min() == -20 and e.max() == 20 and len(set(e.tolist())) == 41
    r0 = _run(w0)
    assert _summary(r0[2]) == WEIGHT_SCALED_SUMMARY and r0[0].tobytes() != sets0.tobytes()  # the weights matter
    for k in (-100, 100):
        g = SR.weight_scaled(k)
        assert (np.ldexp(g.weight.astype(np.float64), -k) == w0.weight).all() and (g.weight >= np.finfo(np.float32).tiny).all() and np.isfinite(g.weight).all()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_run(g), r0))  # every output byte
    g = SR.weight_scaled(SR.SCALE_UNDER)
    s = _run(g)[2]
    assert (_summary(s), int((g.weight == 0).sum()), int(((g.weight > 0) & (g.weight < np.finfo(np.float32).tiny)).sum())) == WEIGHT_UNDER


def test_weights_over_the_whole_range():
    g = SR.weights_range()
    w = g.weight
    assert w.dtype == np.float32 and w[[7, 19, 101, 202]].view(np.uint32).tolist() == [1, 0x7F7FFFFF, 0x80000000, 0]
    e = np.frexp(w[w > 0].astype(np.float64))[1] - 1
    assert e.min() == -149 and e.max() == 127 and np.isfinite(w).all() and (w == 0).sum() == 2 and ((w > 0) & (w < np.finfo(np.float32).tiny)).sum() > 10
    sets, pairs, s = _run(g)
    assert _summary(s, 5) == WEIGHTS_RANGE_SUMMARY and not sets["degenerate"].any() and np.isfinite(sets["X"]).all() and np.isfinite(sets["Rt"]).all()
    assert np.flatnonzero(pairs["used"] == 0).tolist() == [101, 202]


def _hostile_facts(sets, pairs):
    return [int(x) for x in np.flatnonzero(sets["degenerate"])], int((~np.isfinite(sets["Rt"])).sum())


def test_hostile_records_overflow_fp32_under_status_ok():
    """The finding the header now states: every X is finite — |t| up to 4e76 — and 69 components of Rt, X rounded once to fp32, are
    infinite, under status SC_OK."""
    f = SR.hostile()
    assert f.rt.tobytes() == CR.hostile24().rt.tobytes() and np.isfinite(f.rt).all() and (f.pairs == SR.k24().pairs).all()
    for (anchor, max_rounds), (summary, degenerate, not_finite) in HOSTILE.items():
        sets, pairs, s = _run(f, anchor=anchor, max_rounds=max_rounds)
        assert _summary(s, 5) == summary and _hostile_facts(sets, pairs) == (degenerate, not_finite), (anchor, max_rounds)
        assert (sets["degenerate"] <= 1).all() and (sets["status"] == SC_OK).all() and (pairs["status"] == SC_OK).all()
        assert np.isfinite(sets["X"]).all() and 1e76 < np.abs(sets["X"][:, 9:]).max() < 1e77
        assert np.isfinite(pairs["r2"]).all() and np.isfinite(pairs["e2"]).all() and 1e77 < pairs["r2"].max() < 1e79
        assert np.isinf(sets["Rt"][~np.isfinite(sets["Rt"])]).all() and (np.abs(sets["X"])[np.isinf(sets["Rt"])] > CR.FLT_MAX).all()
    # the bite: a result whose Rt stops at +-FLT_MAX where it should be infinite is told apart by the GPU tests' comparison
    from test_gpu_pairs_sync import _assert_same
    exp = _run(f)
    _assert_same(exp, _run(f), "hostile against itself")
    clamped = exp[0].copy()
    clamped["Rt"] = np.clip(exp[0]["Rt"], -SR.FLT_MAX, SR.FLT_MAX)
    assert (clamped["Rt"] != exp[0]["Rt"]).sum() == 69 and np.isfinite(clamped["Rt"]).all()
    try:
        _assert_same((clamped, exp[1], exp[2]), exp, "hostile, Rt clamped")
    except AssertionError as e:
        assert "Rt" in str(e)
    else:
        raise AssertionError("a clamped Rt passes the comparison")


def test_the_ring_of_40_to_the_round_limit():
    f = SR.ring40()
    assert f.n_sets == 40 and len(f.pairs) == 40 and f.params["max_rounds"] == 256
    for (tol, max_rounds), want in RING40.items():
        sets, pairs, s = _run(f, rot_tol=tol, trans_tol=tol, max_rounds=max_rounds)
        assert _summary(s, 5) == want, (tol, max_rounds)
    assert np.flatnonzero(sets["status"] == SC_OK).tolist() == [0, 1, 39]  # one round: the anchor and its two neighbours
    assert 256 - RING40[(1e-4, 256)][0] > 30  # launches that find the stop ahead of them


def test_sparse_is_the_chain_among_sets_with_empty_lists():
    f, c = SR.sparse(), SR.chain()
    assert f.n_sets == SR.WIDE_SETS > 2048 * 4 and (f.pairs == c.pairs).all() and f.rt.tobytes() == c.rt.tobytes()
    assert sorted(set(SR.adjacency(f.pairs)[0].tolist())) == list(range(42)) and f.params["max_rounds"] == 64
    # (a set's round reads its own list and its neighbours: run here among 200 sets, which takes a twentieth of the time; the GPU test
    # runs the reference at 8200 and holds it to the same summary)
    few = SR.sparse(200)
    assert (few.pairs == f.pairs).all() and few.rt.tobytes() == f.rt.tobytes() and few.params == f.params
    sets, pairs, s = _run(few)
    assert _summary(s, 5) == SPARSE_SUMMARY and (sets["status"] == SC_ENOHYP).sum() == 200 - 42
    empty = np.zeros(200 - 42, SR.SET_DTYPE); empty["status"] = SC_ENOHYP
    assert sets[42:].tobytes() == empty.tobytes()  # all zero but the status
    alone = _run(c, max_rounds=64)
    assert sets[:42].tobytes() == alone[0].tobytes() and pairs.tobytes() == alone[1].tobytes() and s.tobytes() == alone[2].tobytes()


def test_a_result_fed_back_as_pose_records():
    for name, (anchor, want) in SELF_STAR.items():
        f = getattr(SR, name)()
        first = _run(f, anchor=anchor)
        g = SR.self_star(first[0], anchor)
        assert g.pairs.tolist() == [[s, anchor] for s in range(f.n_sets)] and g.rt.tobytes() == first[0]["Rt"].tobytes() and g.params["flags"] == SR.STATUS
        sets, pairs, s = _run(g)
        assert _summary(s) == want
        # SC_ENOHYP passes through as the pair's status, and a record that is not finite is SC_EINVAL whatever its status word says
        finite = np.isfinite(first[0]["Rt"]).all(axis=1)
        legal = (first[0]["status"] == SC_OK) & finite
        assert (pairs["status"] == np.where((first[0]["status"] == SC_OK) & ~finite, SC_EINVAL, first[0]["status"])).all()
        assert (sets["status"] == np.where(legal, SC_OK, SC_ENOHYP)).all() and not sets["X"][~legal].any()
        assert pairs["used"].tolist() == [int(ok and s_ != anchor) for s_, ok in enumerate(legal)]
        assert (~legal).sum() == {"k24": 0, "two_components": 6, "hostile": 23}[name]
        if name != "hostile":
            assert np.abs(sets["X"] - first[0]["X"]).max() < 1e-7  # (a sanity note: fp32 rounding and one rot)
