"""CPU suite: the surface of sc_assign_poses (include/saccot.h) — the five exports, the Python mirror, the layouts of sc_assign_params
and sc_assign_result, the default parameters, the argument checks that need no GPU (also under the sanitizers, in a program of their
own) — and the Python restatement of its semantics (tests/assign_ref.py) that the GPU tests compare against: its emulated residual is
pinned to the C restatement bit for bit, and its scenes are checked for what they are used for.  No compute call reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import assign_ref as AR
import instances_batch_ref as IB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_assign_default_params", "sc_assign_poses_frame", "sc_assign_poses_frame_device", "sc_assign_poses_batch",
         "sc_assign_poses_batch_device")
SC_OK, SC_EINVAL = 0, -1
# the truncated score modes in which FIRST on the reference's greedy motions gives the reference peel's scores
# (test_first_on_the_greedy_motions_gives_the_peels_labels_and_scores asserts it for each): the GPU tests compare the scores in these
CONFIRMED_SCORE_MODES = (1, 2)


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_assign_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("assign_poses_frame", "assign_poses_frame_device", "assign_poses_batch", "assign_poses_batch_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.ScAssignParams is pkg.api.ScAssignParams and pkg.ScAssignResult is pkg.api.ScAssignResult and callable(pkg.make_assign_params)
    assert (pkg.SC_ASSIGN_BEST, pkg.SC_ASSIGN_FIRST, pkg.SC_ASSIGN_SEL_NONE, pkg.SC_ASSIGN_SEL_MASK, pkg.SC_ASSIGN_STATUS,
            pkg.SC_ASSIGN_MAX_POSES, pkg.SC_ASSIGN_BATCH_MAX_POSES) == (0, 1, 0, 1, 1, 1024, 64)
    for word in ("slots and pairs forms", "soft or weighted assignment", "relabel and refit until stable", "sharded frames"):
        assert word in header  # what is not here is said


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_ASSIGN 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_assign_struct_layouts_and_constants(pkg):
    exe = os.path.join(ROOT, "tests", ".abi_probe_assign")
    P, R = "sc_assign_params", "sc_assign_result"
    fields = [f"sizeof({P})"] + [f"offsetof({P}, {f})" for f in ("size", "mode", "sel_mode", "flags", "reserved")]
    fields += [f"sizeof({R})"] + [f"offsetof({R}, {f})" for f in ("status", "count", "score", "reserved")]
    consts = ["SC_ASSIGN_BEST", "SC_ASSIGN_FIRST", "SC_ASSIGN_SEL_NONE", "SC_ASSIGN_SEL_MASK", "SC_ASSIGN_STATUS", "SC_ASSIGN_MAX_POSES",
              "SC_ASSIGN_BATCH_MAX_POSES", "SC_HAS_ASSIGN"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("' + "%zu " * len(fields) + "%u " * len(consts)
           + '", ' + ", ".join(fields) + ", " + ", ".join(f"(unsigned){c}" for c in consts) + ");return 0;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    finally:
        os.remove(exe)
    K, Q = pkg.api.ScAssignParams, pkg.api.ScAssignResult
    assert got[:6] == [32, 0, 4, 8, 12, 16]
    assert got[:6] == [C.sizeof(K), K.size.offset, K.mode.offset, K.sel_mode.offset, K.flags.offset, K.reserved.offset]
    assert got[6:11] == [32, 0, 4, 8, 16]
    assert got[6:11] == [C.sizeof(Q), Q.status.offset, Q.count.offset, Q.score.offset, Q.reserved.offset]
    assert got[11:] == [0, 1, 0, 1, 1, 1024, 64, 1]
    for dt in (pkg.ASSIGN_RESULT_DTYPE, AR.RESULT_DTYPE):
        assert dt.itemsize == 32 and [dt.fields[f][1] for f in ("status", "count", "score", "reserved")] == [0, 4, 8, 16]


def test_default_params(pkg):
    L = pkg.load_library()
    ap = pkg.ScAssignParams(1, 2, 3, 4)
    ap.reserved[3] = 9
    assert L.sc_assign_default_params(C.byref(ap)) == SC_OK
    assert bytes(ap) == (32).to_bytes(4, "little") + bytes(28)
    assert L.sc_assign_default_params(None) == SC_EINVAL
    assert bytes(pkg.make_assign_params()) == bytes(ap)
    q = pkg.make_assign_params(mode=pkg.SC_ASSIGN_FIRST, sel_mode=pkg.SC_ASSIGN_SEL_MASK, flags=pkg.SC_ASSIGN_STATUS)
    assert (q.size, q.mode, q.sel_mode, q.flags, list(q.reserved)) == (32, 1, 1, 1, [0, 0, 0, 0])


def test_every_argument_is_refused_without_a_context(pkg):
    L = pkg.load_library()
    ap, p = pkg.make_assign_params(), pkg.make_params()
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on the NULL context before it looks at anything else
    # (a context cannot exist here — sc_create fails without a GPU —; the GPU suites repeat every rule on a real one, where
    # sc_last_error names the reason)
    off = (C.c_uint32 * 2)(0, 8)
    for entry in (L.sc_assign_poses_frame, L.sc_assign_poses_frame_device):
        for stride in (48, 64, 80, 0, 44, 50):
            for n_poses in (1, 0, 1025):
                for d2 in (None, fake):
                    assert entry(None, C.byref(ap), fake, stride, n_poses, None, fake, d2, fake) == SC_EINVAL
        assert entry(None, None, fake, 48, 1, None, fake, None, fake) == SC_EINVAL
        assert entry(None, C.byref(ap), None, 48, 1, None, fake, None, fake) == SC_EINVAL
        assert entry(None, C.byref(ap), fake, 48, 1, None, None, None, fake) == SC_EINVAL
        assert entry(None, C.byref(ap), fake, 48, 1, None, fake, None, None) == SC_EINVAL
        res = pkg.make_assign_params(); res.reserved[1] = 1
        for bad in (pkg.ScAssignParams(31, 0, 0, 0), pkg.make_assign_params(mode=2), pkg.make_assign_params(sel_mode=2),
                    pkg.make_assign_params(sel_mode=1), pkg.make_assign_params(flags=2), res):
            assert entry(None, C.byref(bad), fake, 64, 1, None, fake, None, fake) == SC_EINVAL
    f32 = C.cast(fake, C.POINTER(C.c_float))
    for entry, pts in ((L.sc_assign_poses_batch, f32), (L.sc_assign_poses_batch_device, fake)):
        for stride in (52, 80, 48, 54):
            for n_poses in (1, 0, 65):
                assert entry(None, pts, pts, off, 1, C.byref(p), C.byref(ap), fake, stride, n_poses, fake, fake) == SC_EINVAL
        assert entry(None, None, None, None, 0, None, None, None, 0, 0, None, None) == SC_EINVAL


def test_the_host_checks_under_the_sanitizers(tmp_path):
    """The rules of the parameter block, the stride and n_poses in both forms, the motion-major offsets and the bytes read of the pose
    array: tests/native/assign_check_main.cpp, a program of its own built with -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "assign_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "assign_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


# ---- the reference itself -----------------------------------------------------------------------------------------------------------
def test_the_emulated_fma_rounds_once():
    """cases a plain fp64 add followed by a cast gets wrong, and the ordinary ones"""
    f = np.float32
    a, b, c = f(1 + 2.0**-12), f(1 + 2.0**-12), f(2.0**-60)
    exact = (1 + 2.0**-12) ** 2  # 1 + 2^-11 + 2^-24: a tie of fp32 at 1 + 2^-11 (even) — the addend breaks it upwards
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == f(1 + 2.0**-11)  # the double rounding: wrong
    assert AR.fmaf(a, b, c) == f(1 + 2.0**-11 + 2.0**-23) and exact == 1 + 2.0**-11 + 2.0**-24
    assert AR.fmaf(a, b, -c) == f(1 + 2.0**-11)  # ... and downwards
    assert AR.fmaf(f(3), f(5), f(7)) == f(22) and AR.fmaf(f(3e38), f(10), f(0)) == f(np.inf)
    assert np.isnan(AR.fmaf(f(np.inf), f(0), f(1))) and AR.fmaf(f(1e-30), f(1e-30), f(0)) == f(0)
    rng = np.random.default_rng(5)
    x, y, z = (rng.normal(size=4000).astype(np.float32) for _ in range(3))
    exact = [float(np.float32(float(np.float64(p) * np.float64(q)) + float(r))) for p, q, r in zip(x, y, z)]  # (mostly right; a sanity net)
    assert (AR.fmaf(x, y, z) == np.array(exact, np.float32)).mean() > 0.999


def test_the_emulated_residual_is_the_restatements_bit_for_bit(pkg, O):
    """so_mask on ONE correspondence with tau2 = d2 says 0 (d2 < d2 is false) and with tau2 = nextafter(d2, inf) says 1: the C
    restatement's residual is exactly the emulated one.  A few thousand (pose, m) pairs of the shared scenes, near and far poses."""
    L = O.lib()
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    sc, mo = AR.scene(pkg, 7400), AR.motions(pkg)
    gt = AR.rt_of(sc.R_gt, sc.t_gt)
    poses = list(AR.perturbed(gt, 3, 1)) + [AR.rt_of(*mo.motions[1]), AR.far(gt)]
    rng = np.random.default_rng(11)
    checked = 0
    for scn, rows in ((sc, rng.choice(7400, 500, replace=False)), (mo, rng.choice(1500, 300, replace=False))):
        for Rt in poses:
            d2 = AR.resid2(Rt, scn.src[rows], scn.tgt[rows])
            assert np.isfinite(d2).all()
            rt = np.ascontiguousarray(Rt, np.float32)
            for i, m in enumerate(rows):
                p, q = np.ascontiguousarray(scn.src[m]), np.ascontiguousarray(scn.tgt[m])  # one correspondence: its planes are itself
                out = np.zeros(2, np.uint8)
                for j, thr in enumerate((d2[i], np.nextafter(d2[i], np.float32(np.inf)))):
                    L.so_mask(p.ctypes.data_as(f32p), q.ctypes.data_as(f32p), 1, rt.ctypes.data_as(f32p), C.c_float(float(thr)),
                              out[j:].ctypes.data_as(u8p))
                assert out.tolist() == [0, 1], (m, d2[i])
                checked += 1
    assert checked >= 4000
    # ... and over a whole scene the candidate test is O.mask
    for Rt in poses:
        assert np.array_equal(AR.resid2(Rt, sc.src, sc.tgt) < AR.tau2_of(AR.TAU), O.mask(sc.src, sc.tgt, Rt, AR.TAU).astype(bool))


def test_best_and_first_differ_on_overlapping_poses_and_a_copy_gets_nothing(pkg, O):
    sc = AR.scene(pkg, 7400)
    gt = AR.rt_of(sc.R_gt, sc.t_gt)
    poses = AR.perturbed(gt, 3, 2)
    lb, db, rb = AR.assign(O, sc.src, sc.tgt, poses, AR.TAU, AR.BEST)
    lf, df, rf = AR.assign(O, sc.src, sc.tgt, poses, AR.TAU, AR.FIRST)
    print("BEST", rb["count"].tolist(), "FIRST", rf["count"].tolist())
    assert not np.array_equal(lb, lf) and np.array_equal(lb >= 0, lf >= 0)  # the same correspondences are labelled, differently
    assert (rb["count"] > 0).all() and int(rf["count"][0]) == int(O.mask(sc.src, sc.tgt, poses[0], AR.TAU).sum())
    assert (db[lb >= 0] <= df[lb >= 0]).all() and (db[lb < 0].view(np.uint32) == 0x7F800000).all()
    assert np.array_equal(rb["score"], rb["count"]) and int(rb["count"].sum()) == int((lb >= 0).sum())
    # K = 3 with a duplicate: under BEST the copy never wins its tie; under FIRST it finds everything taken
    dup = np.stack([poses[0], poses[1], poses[0]])
    for mode in (AR.BEST, AR.FIRST):
        lab, _, rec = AR.assign(O, sc.src, sc.tgt, dup, AR.TAU, mode)
        assert int(rec["count"][2]) == 0 and not (lab == 2).any() and int(rec["count"][0]) > 0
    # reversed pose order: BEST's label k becomes K-1-k wherever no two poses tie on the smallest residual
    K = len(poses)
    D = np.stack([AR.resid2(p, sc.src, sc.tgt) for p in poses])
    lr = AR.assign(O, sc.src, sc.tgt, poses[::-1].copy(), AR.TAU, AR.BEST)[0]
    tie = (np.sort(D, axis=0)[0] == np.sort(D, axis=0)[1])
    assert np.array_equal(np.where(lr >= 0, K - 1 - lr, -1)[~tie], lb[~tie]) and (~tie).sum() > 7000
    # the pose lists of the large counts: far poses and the copy claim nothing
    big = AR.many(gt, 65, 3)
    rec = AR.assign(O, sc.src, sc.tgt, big, AR.TAU, AR.BEST)[2]
    assert not rec["count"][3::7].any() and int(rec["count"][5]) == 0 and (rec["count"] > 0).sum() > 20


def test_first_on_the_true_motions_counts_every_labelled_correspondence(pkg, O):
    mo = AR.motions(pkg)
    poses = np.stack([AR.rt_of(R, t) for R, t in mo.motions])
    lab, d2, rec = AR.assign(O, mo.src, mo.tgt, poses, AR.TAU, AR.FIRST)
    assert int(rec["count"].sum()) == int((lab >= 0).sum()) and (rec["count"] >= 100).all() and (rec["status"] == SC_OK).all()
    # a selection: deselected rows are -1 and the records are those of the selected rows alone
    part = np.arange(1500) % 3 != 0
    ls, _, rs = AR.assign(O, mo.src, mo.tgt, poses, AR.TAU, AR.BEST, part)
    l2, _, r2 = AR.assign(O, mo.src[part], mo.tgt[part], poses, AR.TAU, AR.BEST)
    assert (ls[~part] == -1).all() and np.array_equal(ls[part], l2) and rs.tobytes() == r2.tobytes()
    # statuses: passed through, a non-finite pose is SC_EINVAL, neither claims anything, the neighbours keep their records
    bad = poses[0].copy(); bad[3] = np.nan
    four = np.stack([poses[0], poses[1], bad, poses[1]])
    l4, _, r4 = AR.assign(O, mo.src, mo.tgt, four, AR.TAU, AR.FIRST, statuses=[SC_OK, AR.SC_ENOHYP, SC_OK, SC_OK])
    assert r4["status"].tolist() == [SC_OK, AR.SC_ENOHYP, SC_EINVAL, SC_OK] and r4["count"][1:3].tolist() == [0, 0]
    assert np.array_equal(np.where(l4 == 3, 1, l4), lab) and int(r4["count"][3]) == int(rec["count"][1])


def test_first_on_the_greedy_motions_gives_the_peels_labels_and_scores(pkg, O):
    """the reference peel (tests/instances_batch_ref.py::rounds, at any n) against FIRST on its own motions, in every score mode"""
    mo = AR.motions(pkg)
    for score_mode in (0,) + CONFIRMED_SCORE_MODES:
        min_score = 20 if score_mode == 0 else 20 * 1024
        planes, label, found = IB.one(O, mo.src, mo.tgt, dict(AR.kw_of()), score_mode, max_instances=4, min_score=min_score)
        assert found >= 2
        lab, _, rec = AR.assign(O, mo.src, mo.tgt, planes["Rt"][:found], AR.TAU, AR.FIRST, score_mode=score_mode)
        print(score_mode, found, planes["best_count"][:found].tolist(), rec["score"].tolist())
        assert np.array_equal(lab, label)
        assert rec["score"].tolist() == planes["best_count"][:found].tolist(), score_mode
