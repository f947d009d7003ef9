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
    return SR.sync(f.n_sets, f.pairs, f.rt, *thr, **p)


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
