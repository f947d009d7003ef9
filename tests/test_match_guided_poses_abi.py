"""CPU suite: the surface of sc_match_guided_poses (include/saccot.h) — the three exports, the Python mirror, the macros, the argument
checks that need no GPU (also under the sanitizers, in a program of their own) — and the numpy restatement of its semantics
(tests/match_guided_poses_ref.py) that the GPU tests compare against, checked on itself: with one record it is the single-pose
restatement, and the shared scenes have what the GPU tests use them for.  No compute call reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import match_guided_poses_ref as MP
import match_guided_ref as MG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_match_guided_poses_device", "sc_match_guided_poses", "sc_register_guided_poses_features")
SC_OK, SC_EINVAL = 0, -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_poses_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    for method in ("match_guided_poses", "match_guided_poses_device", "register_guided_poses_features"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.SC_GUIDE_MAX_POSES == pkg.api.SC_GUIDE_MAX_POSES == 64
    for word in ("batch and pairs forms of the several-pose gate", "a gate radius per pose", "per-pose tallies (sc_assign_poses_frame counts",
                 "soft weighting by the residuals", "several poses per call (entries of their own: sc_match_guided_poses", "several poses per problem"):
        assert word in header  # what is not here is said, and where the frame form's several poses are


def test_the_minor_version_stays_and_the_macros_are_visible_from_c(pkg, tmp_path):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_MATCH_GUIDED_POSES 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10
    exe = str(tmp_path / "abi_probe_match_guided_poses")
    src = ('#include <stdio.h>\n#include "saccot.h"\nint main(void){printf("%u %u %u", (unsigned)SC_HAS_MATCH_GUIDED_POSES, '
           '(unsigned)SC_GUIDE_MAX_POSES, (unsigned)SC_GUIDE_POSE_STATUS);return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    assert subprocess.check_output([exe]).decode().split() == ["1", "64", "1"]


def test_every_entry_is_refused_without_a_context(pkg):
    L = pkg.load_library()
    mp, gp, p = pkg.api.make_match_params(8), pkg.make_guide_params(0.1), pkg.make_params()
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on the NULL context before it looks at anything else
    f32 = C.cast(fake, C.POINTER(C.c_float))
    i32, u8 = C.cast(fake, C.POINTER(C.c_int32)), C.cast(fake, C.POINTER(C.c_uint8))
    assert L.sc_match_guided_poses_device(None, fake, fake, 4, fake, fake, 4, C.byref(mp), C.byref(gp), fake, 48, 1, fake, fake, fake, fake,
                                          fake) == SC_EINVAL
    assert L.sc_match_guided_poses_device(None, None, None, 0, None, None, 0, None, None, None, 0, 0, None, None, None, None, None) == SC_EINVAL
    n = C.c_uint32(7)
    assert L.sc_match_guided_poses(None, f32, f32, 4, f32, f32, 4, C.byref(mp), C.byref(gp), fake, 48, 1, i32, f32, f32, i32,
                                   C.byref(n)) == SC_EINVAL
    assert n.value == 0
    assert L.sc_match_guided_poses(None, None, None, 0, None, None, 0, None, None, None, 0, 0, None, None, None, None, None) == SC_EINVAL
    n = C.c_uint32(7)
    assert L.sc_register_guided_poses_features(None, f32, f32, 4, f32, f32, 4, C.byref(mp), C.byref(gp), fake, 48, 65, C.byref(p), f32, f32,
                                               i32, f32, f32, i32, C.byref(n), u8, None) == SC_EINVAL
    assert n.value == 0
    assert L.sc_register_guided_poses_features(None, None, None, 0, None, None, 0, None, None, None, 0, 0, None, None, None, None, None,
                                               None, None, None, None, None) == SC_EINVAL


def test_the_host_checks_under_the_sanitizers(tmp_path):
    """The stride (44, 46, 50; 48 with the flag), n_poses 0 and 65, an unknown flag, every rule of sc_guide_params and their order:
    tests/native/match_guided_poses_check_main.cpp, a program of its own built with -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "match_guided_poses_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "match_guided_poses_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


# ---- the restatement checked on itself -----------------------------------------------------------------------------------------------
def test_one_record_is_the_single_pose_restatement():
    for ns, nt, D in ((130, 129, 33), (3, 5, 1), (1, 1, 1)):
        sc = MP.shared_scene(ns, nt, D, 1)
        prob, one = MP.Problem(*sc.args(), MP.GATE), MG.Problem(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, sc.poses[0], MP.GATE)
        for kw in MG.MODES:
            c, d, g, lab = prob.match(**kw)
            ec, ed, eg = one.match(**kw)
            assert c.tobytes() == ec.tobytes() and d.tobytes() == ed.tobytes() and g.tobytes() == eg.tobytes() and not lab.any(), (ns, nt, D, kw)


def test_the_shared_scene_has_what_the_gpu_tests_use_it_for():
    sc = MP.shared_scene(300, 333, 33, 3)
    prob = MP.Problem(*sc.args(), MP.GATE)
    singles = [MG.Problem(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, sc.poses[k], MP.GATE) for k in range(3)]
    gate2 = MG.gate2_of(MP.GATE)
    for kw in MG.MODES:
        c, d, g, lab = prob.match(**kw)
        print(kw, "n", len(c), "per record", np.bincount(lab, minlength=3).tolist())
        assert (np.bincount(lab, minlength=3) > 0).all(), kw  # every record labels at least one entry
        assert (g < gate2).all() and prob.adm[c[:, 0], c[:, 1]].all(), kw
        rows = set(map(tuple, c.tolist()))
        alone = [set(map(tuple, s.match(**kw)[0].tolist())) for s in singles]
        # the union is none of the single-pose calls: for every record some output row is not in that record's result
        assert all(rows - a for a in alone), kw
        # ... and not their concatenation either: a row re-assigned under the union is in NO single-pose result only if the tests
        # of mutual / ratio saw other candidates; what must hold is that the label's record admits the entry with that residual
        for k in range(3):
            sel = lab == k
            assert singles[k].adm[c[sel, 0], c[sel, 1]].all() and g[sel].tobytes() == singles[k].g2[c[sel, 0], c[sel, 1]].tobytes(), (kw, k)
    # the status flag: a record that is not used takes no part
    c, d, g, lab = MP.Problem(*sc.args(), MP.GATE, used=[True, False, True]).match(knn=2)
    assert set(np.unique(lab)) == {0, 2}
    assert len(MP.Problem(*sc.args(), MP.GATE, used=[False] * 3).match(knn=4)[0]) == 0


def test_the_tie_scene_never_yields_the_higher_index():
    sc = MP.tie_scene(300, 333, 33)
    assert sc.poses[0].tobytes() == sc.poses[1].tobytes()
    for kw in MG.MODES:
        lab = MP.match(*sc.args(), MP.GATE, **kw)[3]
        assert len(lab) and (lab != 1).all() and (lab == 0).any() and (lab == 2).any(), kw


def test_the_cluster_scenes_drop_the_tiles_the_gpu_tests_say_they_drop():
    sc = MP.cluster_scene()
    prob = MP.Problem(*sc.args(), MP.GATE)
    tiles = [slice(0, 64), slice(64, 128), slice(128, 129)]
    per = np.array([[prob.adm_k[k][:, t].any() for t in tiles] for k in range(3)])
    print(per.astype(int))
    assert per.tolist() == [[True, False, False], [False, False, False], [False, True, False]]  # tile 1: record 2 only; tile 2: none
    c, _, _, lab = prob.match(knn=4)
    assert set(np.unique(lab)) == {0, 2} and len(c) == 4 * 130
    big = MP.two_tiles_scene()
    prob = MP.Problem(*big.args(), MP.GATE)
    col_tiles = np.unique(np.flatnonzero(prob.adm.any(axis=0)) // 64)
    assert len(col_tiles) > 600 and (col_tiles % 3 != 2).all() and not prob.adm_k[1].any()
    only2 = np.unique(np.flatnonzero(prob.adm_k[2].any(axis=0)) // 64)
    assert (only2 % 3 == 1).all() and not prob.adm_k[0][:, prob.adm_k[2].any(axis=0)].any()
