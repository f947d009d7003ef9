"""CPU suite: the surface of sc_pairs_solve (include/saccot.h) — the four exports, the Python mirror, the layouts of sc_solve_params,
sc_solve_set, sc_solve_pair and sc_solve_summary compiled in C99, the default parameters, sc_solve_thresholds, every rule that refuses
a call with its text (the host-only rules run under the sanitizers, in a program of their own) — and the Python restatement
(tests/solve_ref.py) that the GPU tests compare against: it is held to a dense solver it shares no code with, and its input families
are checked for what they are used for.  No compute call reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import solve_ref as V
import sync_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_solve_default_params", "sc_solve_thresholds", "sc_pairs_solve", "sc_pairs_solve_device")
SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def _section():
    header = _header()
    return header[header.index("sc_pairs_solve ---"):header.index("two-phase form for one-process-per-GPU sharding")]


def test_solve_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    for method in ("pairs_solve", "pairs_solve_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert callable(pkg.make_solve_params) and callable(pkg.solve_thresholds)
    for struct, dtype, ref in (("ScSolveSet", "SOLVE_SET_DTYPE", V.SET_DTYPE), ("ScSolvePair", "SOLVE_PAIR_DTYPE", V.PAIR_DTYPE),
                               ("ScSolveSummary", "SOLVE_SUMMARY_DTYPE", V.SUMMARY_DTYPE)):
        S, D = getattr(pkg, struct), getattr(pkg, dtype)
        assert np.dtype(S) == D and D.itemsize == C.sizeof(S) == ref.itemsize and list(D.names) == list(ref.names)
        assert [D.fields[f][1] for f in D.names] == [ref.fields[f][1] for f in ref.names] == [getattr(S, f).offset for f in D.names]
        assert [D.fields[f][0] for f in D.names] == [ref.fields[f][0] for f in ref.names]
    assert (pkg.SC_SOLVE_STATUS, pkg.SC_SOLVE_INFO_STATUS) == (V.STATUS, V.INFO_STATUS) == (1, 2)
    assert (pkg.SC_SOLVE_FREE, pkg.SC_SOLVE_ANCHOR, pkg.SC_SOLVE_UNKNOWN, pkg.SC_SOLVE_ISOLATED) == (V.FREE, V.ANCHOR, V.UNKNOWN, V.ISOLATED) == (0, 1, 2, 3)
    assert (pkg.SC_SOLVE_STOP_CONVERGED, pkg.SC_SOLVE_STOP_ROSE, pkg.SC_SOLVE_STOP_MAX_OUTER) == (V.CONVERGED, V.ROSE, V.MAX_OUTER) == (1, 2, 3)
    # an init record is what sc_pairs_sync and the entry itself write; an info record what sc_pose_info writes
    for D in (pkg.SYNC_SET_DTYPE, pkg.SOLVE_SET_DTYPE):
        assert D.itemsize == 160 and D.fields["status"][1] == 48 and D.fields["X"][1] == 64
    assert pkg.POSE_INFO_RESULT_DTYPE.itemsize == 320 == V.INFO_DTYPE.itemsize and pkg.POSE_INFO_RESULT_DTYPE.fields["status"][1] == 296
    assert pkg.POSE_INFO_RESULT_DTYPE.fields["info"][1] == 0


def test_the_minor_version_stays_and_the_sync_section_points_here(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_PAIRS_SOLVE 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10
    assert header.index("sc_pairs_solve ---") > header.index("sc_pairs_sync ---")
    sync = " ".join(header[header.index("sc_pairs_sync ---"):header.index("sc_pairs_solve ---")].replace("\n * ", "\n").split())
    assert "is sc_pairs_solve (below)" in sync and "not built: a block solver" not in sync


def test_the_section_states_the_method_and_every_rule():
    flat = " ".join(_section().replace("\n * ", "\n").split())
    for word in ("Not here / not built:", "Levenberg-Marquardt damping", "robust re-weighting", "a one-workgroup form for small graphs", "several anchors",
                 "a sharded form", "solved only up to its own gauge", "SC_SOLVE_STOP_ROSE", "no NaN is ever written into X", "the finite guards above are built"):
        assert word in flat, word
    for rule in ("E = D o T_p(b->a)", "omega_0 = (E.R_21 - E.R_12) / 2.0", "y_i = sum_j info[6 i + j] * xi_j", "cost_p = sum_i xi_i * y_i",
                 "A[3 + i][j] = -(c x t)_j", "W[i][j] = W[j][i] = sum_k A[k][i] * M[k][j] for i <= j", "g_i = sum_k A[k][i] * y_k",
                 "H_aa += W_p, H_bb += W_p, H_ab = H_ba = -W_p", "e_j = d(s)_j - d(n)_j", "L_ij = a / D_j", "z_i = z_i - L_ki * z_k",
                 "chunks of 64 consecutive sets", "beta = rz_{i-1} / rz_{i-2}, p_c = z_c + beta * p_c", "alpha = rz_{i-1} / pq",
                 "rz_i <= cg2 * rz_0", "Q = rot(I + [omega]x)", "R' = rot(Q R)", "If !(c_j <= c_{j-1})", "cg2 = (double)cg_tol * (double)cg_tol",
                 "5 + max_outer * (4 + 2 * max_inner) launches", "max_outer * max_inner > 2048"):
        assert rule in flat, rule
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "sc_pairs_solve_device" in integration
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "solve_product_kernel" in design


def test_the_struct_layouts_and_the_macros_in_c(pkg, tmp_path):
    exe = str(tmp_path / "solve_layout")
    P, S, R, M = "sc_solve_params", "sc_solve_set", "sc_solve_pair", "sc_solve_summary"
    pf = ("size", "anchor", "max_outer", "max_inner", "flags", "rot_tol", "trans_tol", "cg_tol")
    sf = ("Rt", "status", "state", "degenerate", "reserved", "X")
    rf = ("status", "used", "cost", "w2", "v2", "reserved")
    mf = ("outer", "stop", "inner_total", "inner_last", "free_sets", "used_pairs", "held_last", "reserved", "cost0", "cost", "rz0", "reserved2")
    fields = []
    for name, fs in ((P, pf), (S, sf), (R, rf), (M, mf)):
        fields += [f"sizeof({name})"] + [f"offsetof({name}, {f})" for f in fs]
    consts = ["SC_SOLVE_STATUS", "SC_SOLVE_INFO_STATUS", "SC_HAS_PAIRS_SOLVE", "SC_SOLVE_FREE", "SC_SOLVE_ANCHOR", "SC_SOLVE_UNKNOWN", "SC_SOLVE_ISOLATED",
              "SC_SOLVE_STOP_CONVERGED", "SC_SOLVE_STOP_ROSE", "SC_SOLVE_STOP_MAX_OUTER"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("' + "%zu " * len(fields) + "%u " * len(consts)
           + '", ' + ", ".join(fields) + ", " + ", ".join(f"(unsigned){c}" for c in consts) + ");return 0;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[:9] == [32, 0, 4, 8, 12, 16, 20, 24, 28] == [C.sizeof(pkg.ScSolveParams)] + [getattr(pkg.ScSolveParams, f).offset for f in pf]
    assert got[9:16] == [160, 0, 48, 52, 56, 60, 64] == [C.sizeof(pkg.ScSolveSet)] + [getattr(pkg.ScSolveSet, f).offset for f in sf]
    assert got[16:23] == [48, 0, 4, 8, 16, 24, 32] == [C.sizeof(pkg.ScSolvePair)] + [getattr(pkg.ScSolvePair, f).offset for f in rf]
    assert got[23:36] == [64, 0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56] == [C.sizeof(pkg.ScSolveSummary)] + [getattr(pkg.ScSolveSummary, f).offset for f in mf]
    assert got[36:] == [1, 2, 1, 0, 1, 2, 3, 1, 2, 3]


def test_default_params_and_null_arguments(pkg):
    L = pkg.load_library()
    sp = pkg.ScSolveParams()
    sp.cg_tol = 0.5; sp.rot_tol = 0.5; sp.flags = 1; sp.anchor = 7
    assert L.sc_solve_default_params(C.byref(sp)) == SC_OK
    assert (sp.size, sp.anchor, sp.max_outer, sp.max_inner, sp.flags, sp.rot_tol, sp.trans_tol, sp.cg_tol) == (32, 0, 8, 64, 0, 0.0, 0.0, 0.0)
    assert L.sc_solve_default_params(None) == SC_EINVAL
    assert bytes(pkg.make_solve_params()) == bytes(sp)  # the Python defaults are the library's
    mk = pkg.make_solve_params(0.25, 0.5, 0.125, anchor=3, max_outer=7, max_inner=9, flags=3)
    assert (mk.size, mk.anchor, mk.max_outer, mk.max_inner, mk.flags, mk.rot_tol, mk.trans_tol, mk.cg_tol) == (32, 3, 7, 9, 3, 0.25, 0.5, 0.125)
    # (a context cannot exist here — sc_create fails without a GPU — so the NULL context is what is tried; the GPU suite tries the
    # rest with a context and reads sc_last_error, and the program below checks every rule's text)
    pairs = (C.c_uint32 * 2)(0, 1)
    assert L.sc_pairs_solve(None, 2, pairs, 1, C.byref(mk), None, 48, None, 4, None, 288, None, 160, None, None, None) == SC_EINVAL
    assert L.sc_pairs_solve_device(None, 2, pairs, 1, C.byref(mk), None, 48, None, 4, None, 288, None, 160, None, None, None) == SC_EINVAL


def test_the_thresholds(pkg):
    L = pkg.load_library()
    out, two = (C.c_double * 3)(), (C.c_double * 2)()
    for rot, trans, cg in ((0.0, 0.0, 0.0), (1e-6, 1e-6, 1e-3), (0.25, 0.5, 0.125), (1.0, 3.0, 0.9), (3.1415927, 1e19, 0.99999994), (1e-8, 1e-20, 1e-30)):
        sp = pkg.make_solve_params(rot, trans, cg)
        assert L.sc_solve_thresholds(C.byref(sp), out) == SC_OK
        cg32 = float(np.float32(cg))
        assert out[2] == cg32 * cg32  # exactly: one product
        yp = pkg.make_sync_params(rot, trans)
        assert L.sc_sync_thresholds(C.byref(yp), two) == SC_OK and (out[0], out[1]) == (two[0], two[1])  # sc_sync_thresholds' two values
        assert pkg.solve_thresholds(sp) == (out[0], out[1], out[2]) == V.thresholds(rot, trans, cg)
    assert L.sc_solve_thresholds(None, out) == SC_EINVAL and L.sc_solve_thresholds(C.byref(sp), None) == SC_EINVAL
    for bad in (pkg.make_solve_params(-0.1), pkg.make_solve_params(3.2), pkg.make_solve_params(0.1, -1.0), pkg.make_solve_params(float("nan")),
                pkg.make_solve_params(0.1, float("inf")), pkg.make_solve_params(0.1, 0.1, 1.0), pkg.make_solve_params(0.1, 0.1, -0.1),
                pkg.make_solve_params(0.1, 0.1, float("nan")), pkg.make_solve_params(max_outer=33), pkg.make_solve_params(max_outer=0),
                pkg.make_solve_params(max_inner=257), pkg.make_solve_params(max_inner=0), pkg.make_solve_params(max_outer=9, max_inner=256),
                pkg.make_solve_params(flags=4)):
        assert L.sc_solve_thresholds(C.byref(bad), out) == SC_EINVAL
    wrong = pkg.make_solve_params(0.1, 0.1); wrong.size = 28
    assert L.sc_solve_thresholds(C.byref(wrong), out) == SC_EINVAL


def test_the_host_rules_under_the_sanitizers(tmp_path):
    """Every refusal rule of sc_solve_check.hpp with its text, the thresholds, the bytes read of the strided info and init arrays and
    the workspace offsets: tests/native/solve_check_main.cpp, a program of its own built with -fsanitize=address,undefined and run on
    the CPU."""
    exe = str(tmp_path / "solve_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "solve_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


# ---- the reference is held to a dense solver it shares no code with -----------------------------------------------------------------
def _exp(d):
    """exp of a twist (omega, v) as a 4 x 4 matrix: Rodrigues' rotation, and v as the translation (the two agree with the group's
    exponential to first order, which is all a Jacobian at 0 and a retraction need)"""
    w = d[:3]
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) if th < 1e-300 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, d[3:]
    return T


def _dense_optimum(f, X0, anchor=0, steps=30):
    """Gauss-Newton with a DENSE normal matrix, a Jacobian by central differences of the error itself, numpy.linalg.solve and matrix
    products throughout, iterated until the cost no longer falls -> the cost at the fixed point.  Nothing of solve_ref is used."""
    n, P = f.n_sets, len(f.pairs)
    T = [np.eye(4) for _ in range(P)]
    for p in range(P):
        T[p][:3, :3], T[p][:3, 3] = f.rt[p, :9].astype(np.float64).reshape(3, 3), f.rt[p, 9:].astype(np.float64)
    Tinv = [np.linalg.inv(t) for t in T]
    info = [np.eye(6) if f.info is None else f.info[p].reshape(6, 6) for p in range(P)]
    X = []
    for s in range(n):
        M = np.eye(4); M[:3, :3], M[:3, 3] = X0[s, :9].reshape(3, 3), X0[s, 9:]
        X.append(M)

    def xi(p, Xa, Xb):
        E = np.linalg.inv(Xb) @ Xa @ Tinv[p]
        return np.array([(E[2, 1] - E[1, 2]) / 2, (E[0, 2] - E[2, 0]) / 2, (E[1, 0] - E[0, 1]) / 2, E[0, 3], E[1, 3], E[2, 3]])

    def cost(X):
        return sum(float(xi(p, X[a], X[b]) @ info[p] @ xi(p, X[a], X[b])) for p, (a, b) in enumerate(f.pairs.tolist()))

    free = [s for s in range(n) if s != anchor]
    col = {s: 6 * k for k, s in enumerate(free)}
    h = 1e-6
    c = cost(X)
    for _ in range(steps):
        H, g = np.zeros((6 * len(free), 6 * len(free))), np.zeros(6 * len(free))
        for p, (a, b) in enumerate(f.pairs.tolist()):
            r = xi(p, X[a], X[b])
            J = {}
            for s in (a, b):
                Js = np.zeros((6, 6))
                for k in range(6):
                    d = np.zeros(6); d[k] = h
                    plus = xi(p, _exp(d) @ X[a] if s == a else X[a], _exp(d) @ X[b] if s == b else X[b])
                    minus = xi(p, _exp(-d) @ X[a] if s == a else X[a], _exp(-d) @ X[b] if s == b else X[b])
                    Js[:, k] = (plus - minus) / (2 * h)
                J[s] = Js
            for s in (a, b):
                if s == anchor:
                    continue
                g[col[s]:col[s] + 6] += J[s].T @ info[p] @ r
                for u in (a, b):
                    if u != anchor:
                        H[col[s]:col[s] + 6, col[u]:col[u] + 6] += J[s].T @ info[p] @ J[u]
        d = np.linalg.solve(H, -g)
        Xn = list(X)
        for s in free:
            Xn[s] = _exp(d[col[s]:col[s] + 6]) @ X[s]
        cn = cost(Xn)
        if not cn < c:
            break
        X, c = Xn, cn
    return c


def test_the_reference_reaches_the_dense_optimum():
    """The reference's final cost at the default parameters against the fixed point of an independent dense Gauss-Newton (a full
    Jacobian by central differences, numpy.linalg.solve) from the same start, noise 0.01 rad / 0.02 units, info from 100 points a pair.
    Measured relative gaps (reference - dense) / dense, and the start's:
      ring of 40          7.4e-6   (reference 0.01039485188229, dense 0.01039477477886; start 7.1)
      24 sets, all pairs  1.5e-6   (reference 4.79167060061450, dense 4.79166356220302; start 0.040)
    The bounds are ten times these: 7.4e-5 and 1.5e-5.  The gap is the method's, not rounding's: Gauss-Newton drops the dependence of
    xi's Jacobian on xi, so its fixed point is where ITS gradient vanishes, second order in the residual away from the dense
    solver's.  A wrong sign or a wrong Jacobian leaves the cost orders of magnitude away — the first step raises the cost, the call
    stops with ROSE at the start's cost, a gap of 7.1 and 0.040 —; the bounds do not guard rounding."""
    bounds = {"ring40": 7.4e-5, "k24": 1.5e-5}
    for name, f in (("ring40", V.ring40()), ("k24", V.k24())):
        X0, st0 = V.sync_start(f)
        _sets, _res, s = V.run(f, init=(X0, st0))
        dense = _dense_optimum(f, X0)
        gap = (float(s["cost"]) - dense) / dense
        print(name, "reference", repr(float(s["cost"])), "dense", repr(dense), "gap", gap, "start", float(s["cost0"]))
        assert int(s["stop"]) == V.CONVERGED and abs(gap) <= bounds[name], (name, gap)
        assert (float(s["cost0"]) - dense) / dense > 0.04  # the start is far from it: the solve did the work


def test_the_solve_converges_where_the_rounds_do_not():
    """The reason for the entry, on the references alone: on the ring of 40 sync_ref.sync at its largest max_rounds (256) and tolerance
    1e-6 does not converge; solve_ref started from that same result stops CONVERGED at 1e-6."""
    f = V.ring40()
    r2, e2 = SR.thresholds(1e-6, 1e-6)
    sets, _res, s = SR.sync(f.n_sets, f.pairs, f.rt, r2, e2, max_rounds=256)
    assert (int(s["rounds"]), int(s["converged"])) == (256, 0) and int(s["changed_last"]) > 0
    tr = []
    q = f.params
    thr = V.thresholds(1e-6, 1e-6, q["cg_tol"])
    _sets, _pairs, v = V.solve(f.n_sets, f.pairs, f.rt, sets["X"], sets["status"], *thr, info=f.info, trace=tr)
    print(v, tr)
    assert (int(v["stop"]), int(v["outer"]), int(v["inner_total"])) == (V.CONVERGED, 5, 320) and float(v["cost"]) < 0.0104 < 0.0232 < float(v["cost0"])


def test_the_families_are_what_they_are_used_for():
    f = V.exact24()
    sets, res, s = V.run(f, init=(f.init_X, f.init_status))
    assert sets["X"].tobytes() == f.init_X.tobytes() and (int(s["outer"]), int(s["stop"]), int(s["inner_total"])) == (1, V.CONVERGED, 0)
    assert float(s["cost"]) == 0.0 and float(s["rz0"]) == 0.0 and not res["cost"].any()
    g = V.k24(V.ROSE_RAD, V.ROSE_TRANS)
    assert int(V.run(g, max_outer=32, rot_tol=0.0, trans_tol=0.0)[2]["stop"]) == V.ROSE
    assert int(V.run(V.k24(), max_outer=1)[2]["stop"]) == V.MAX_OUTER and int(V.run(V.k24())[2]["inner_last"]) == 13
    h = V.held()
    sets, _res, s = V.run(h)
    assert int(s["held_last"]) == 1 and int(sets["degenerate"][4]) == int(s["outer"]) and sets["X"][4].tobytes() == V.sync_start(h)[0][4].tobytes()
    e = V.edges()
    sets, res, s = V.run(e, init=(e.init_X, e.init_status))
    assert int(s["free_sets"]) == 21 and sets["state"][[3, 5, 7]].tolist() == [V.ANCHOR, V.UNKNOWN, V.UNKNOWN]
    assert np.isnan(sets["X"][7, 4]) and np.isfinite(np.delete(sets["X"], 7, axis=0)).all()  # passed through; no NaN is ever written
    for n in (66, 130):
        assert (V.hub(n).pairs == 0).any(axis=1).sum() == n - 1
    fl = V.floating()
    assert int(V.run(fl, init=(fl.init_X, fl.init_status))[2]["free_sets"]) == 29
    # a NULL info and identity records are the same call
    k = V.k24(info=False)
    ident = V.Family(24, k.pairs, k.rt, np.tile(np.eye(6).ravel(), (276, 1)))
    a, b = V.run(k), V.run(ident)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_the_strip_of_200():
    """The numbers of the header's limits paragraph: the odometry strip of 200 sets with 40 closures, started from 256 rounds of
    sync_ref.sync at 1e-6 (unconverged: 199 sets changed in the last).  At the defaults 4 steps of 64 iterations are kept, cost 0.7261 ->
    0.410234, and the fifth rises in the last digits (ROSE); at max_inner 256 the call stops CONVERGED after 4 steps and 510
    iterations at 0.410233571; the dense solver of this file finds 0.410230188."""
    f = V.strip200()
    X0, st0 = V.sync_start(f, max_rounds=256, tol=1e-6)
    tr = []
    q = f.params
    thr = V.thresholds(q["rot_tol"], q["trans_tol"], q["cg_tol"])
    _sets, _pairs, s = V.solve(f.n_sets, f.pairs, f.rt, X0, st0, *thr, info=f.info, trace=tr)
    print(s, tr)
    assert (int(s["outer"]), int(s["stop"]), int(s["inner_total"])) == (4, V.ROSE, 320) and 0.4102 < float(s["cost"]) < 0.4103 < 0.72 < float(s["cost0"])
    _sets, _pairs, s = V.solve(f.n_sets, f.pairs, f.rt, X0, st0, *thr, info=f.info, max_inner=256)
    assert (int(s["outer"]), int(s["stop"]), int(s["inner_total"])) == (4, V.CONVERGED, 510) and 0.4102 < float(s["cost"]) < 0.4103
