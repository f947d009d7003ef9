"""CPU suite: the surface of sc_merge_poses (include/saccot.h) — the five exports, the Python mirror, the layouts of sc_merge_params
and sc_merge_pose, the default parameters, the macros, the argument checks that need no GPU (also under the sanitizers, in a program
of their own) — and the Python restatement of its semantics (tests/merge_ref.py) that the GPU tests compare against: its pose lists
are checked for what they are used for, and the equalities the header promises hold on the references themselves.  No compute call
reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import merge_ref as MR
import polish_poses_ref as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_merge_default_params", "sc_merge_poses_frame", "sc_merge_poses_frame_device", "sc_merge_poses_batch",
         "sc_merge_poses_batch_device")
SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
FRACTIONS = ((1, 1), (1, 2), (1, 8))


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_merge_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    for method in ("merge_poses_frame", "merge_poses_frame_device", "merge_poses_batch", "merge_poses_batch_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.ScMergeParams is pkg.api.ScMergeParams and pkg.ScMergePose is pkg.api.ScMergePose and callable(pkg.make_merge_params)
    assert pkg.MERGE_POSE_DTYPE == np.dtype(pkg.ScMergePose) == MR.POSE_DTYPE and pkg.MERGE_POSE_DTYPE.itemsize == 64
    assert [pkg.MERGE_POSE_DTYPE.fields[f][1] for f in ("Rt", "status", "index", "count", "score")] == [0, 48, 52, 56, 60]
    assert (pkg.SC_MERGE_MAX_POSES, pkg.SC_MERGE_BATCH_MAX_POSES, pkg.SC_MERGE_OVER_MIN, pkg.SC_MERGE_OVER_UNION, pkg.SC_MERGE_STATUS,
            pkg.SC_MERGE_COMPACT) == (1024, 64, 0, 1, 1, 2)
    assert (MR.OVER_MIN, MR.OVER_UNION, MR.STATUS, MR.COMPACT) == (0, 1, 1, 2)


def test_the_two_not_here_pointers(pkg):
    header = _header()
    settle = header[header.index("sc_settle_poses ---"):header.index("sc_merge_poses ---")]
    assert "Not here: merging or dropping poses (an entry of its own: sc_merge_poses, below)" in settle
    for word in ("two copies of a pose split its inliers", "soft assignment", "slots and pairs forms", "sharded frames"):
        assert word in settle  # every phrase that was there is still there
    assign = header[header.index("sc_assign_poses ---"):header.index("sc_settle_poses ---")]
    assert "(an entry of its own: sc_merge_poses, below)" in assign and "sc_settle_poses, below" in assign
    block = header[header.index("sc_merge_poses ---"):]
    for word in ("Not here:", "a refit of the kept poses", "slots and pairs forms", "sharded frames"):
        assert word in block


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_MERGE 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_the_struct_layouts_and_the_macros_in_c(pkg, tmp_path):
    exe = str(tmp_path / "merge_layout")
    P, R = "sc_merge_params", "sc_merge_pose"
    fields = ([f"sizeof({P})"] + [f"offsetof({P}, {f})" for f in ("size", "measure", "num", "den", "min_count", "sel_mode", "flags", "reserved")]
              + [f"sizeof({R})"] + [f"offsetof({R}, {f})" for f in ("Rt", "status", "index", "count", "score")])
    consts = ["SC_MERGE_MAX_POSES", "SC_MERGE_BATCH_MAX_POSES", "SC_MERGE_OVER_MIN", "SC_MERGE_OVER_UNION", "SC_MERGE_STATUS",
              "SC_MERGE_COMPACT", "SC_HAS_MERGE", "SC_ASSIGN_BATCH_MAX_POSES"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("' + "%zu " * len(fields) + "%u " * len(consts)
           + '", ' + ", ".join(fields) + ", " + ", ".join(f"(unsigned){c}" for c in consts) + ");return 0;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    K, Q = pkg.api.ScMergeParams, pkg.api.ScMergePose
    assert got[:9] == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    assert got[:9] == [C.sizeof(K)] + [getattr(K, f).offset for f in ("size", "measure", "num", "den", "min_count", "sel_mode", "flags", "reserved")]
    assert got[9:15] == [64, 0, 48, 52, 56, 60]
    assert got[9:15] == [C.sizeof(Q)] + [getattr(Q, f).offset for f in ("Rt", "status", "index", "count", "score")]
    assert got[15:] == [1024, 64, 0, 1, 1, 2, 1, 64]


def test_default_params_and_null_arguments(pkg):
    L = pkg.load_library()
    mp = pkg.ScMergeParams()
    mp.reserved[0] = 9
    mp.min_count = 4
    assert L.sc_merge_default_params(C.byref(mp)) == SC_OK
    assert (mp.size, mp.measure, mp.num, mp.den, mp.min_count, mp.sel_mode, mp.flags, list(mp.reserved)) == (32, 0, 1, 2, 0, 0, 0, [0])
    assert L.sc_merge_default_params(None) == SC_EINVAL
    mk = pkg.make_merge_params()
    assert bytes(mk) == bytes(mp)  # the Python defaults are the library's
    mk = pkg.make_merge_params(measure=1, num=3, den=4, min_count=5, sel_mode=1, flags=3)
    assert (mk.size, mk.measure, mk.num, mk.den, mk.min_count, mk.sel_mode, mk.flags) == (32, 1, 3, 4, 5, 1, 3)
    # a NULL context is refused before anything is touched, in all four entries
    assert L.sc_merge_poses_frame(None, C.byref(mp), None, 48, 1, None, None, None, None, None) == SC_EINVAL
    assert L.sc_merge_poses_frame_device(None, C.byref(mp), None, 48, 1, None, None, None, None, None) == SC_EINVAL
    assert L.sc_merge_poses_batch(None, None, None, None, 0, None, None, None, 0, 0, None, None, None) == SC_EINVAL
    assert L.sc_merge_poses_batch_device(None, None, None, None, 0, None, None, None, 0, 0, None, None, None) == SC_EINVAL


def test_the_host_checks_under_the_sanitizers(tmp_path):
    """Every refusal rule of sc_merge_check.hpp, the bytes read of the pose array and the scratch sizes:
    tests/native/merge_check_main.cpp, a program of its own built with -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "merge_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "merge_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


# ---- the reference itself: the pose lists are what they are used for ---------------------------------------------------------------
def _merged(pkg, O, name, **kw):
    mo = MR.motions(pkg)
    out = MR.merge(O, mo.src, mo.tgt, MR.lists(pkg)[name], MR.TAU, **kw)
    print(name, kw, "kept, valid", out[3].tolist(), "parent", out[1].tolist(), "count", out[0]["count"].tolist(), "score", out[0]["score"].tolist())
    return out


def test_the_pose_lists_merge_as_the_gpu_tests_need_them_to(pkg, O):
    # near: the fraction matters, and so does the measure
    kept = {(m, f): int(_merged(pkg, O, "near", measure=m, num=f[0], den=f[1])[3][0]) for m in (MR.OVER_MIN, MR.OVER_UNION) for f in FRACTIONS}
    assert len({kept[(MR.OVER_MIN, f)] for f in FRACTIONS}) >= 2
    only_min = False
    for f in FRACTIONS:
        a = _merged(pkg, O, "near", measure=MR.OVER_MIN, num=f[0], den=f[1])[1]
        b = _merged(pkg, O, "near", measure=MR.OVER_UNION, num=f[0], den=f[1])[1]
        only_min = only_min or any(a[k] != k and b[k] == k for k in range(len(a)))
    assert only_min  # a fold under OVER_MIN that OVER_UNION does not make at the same fraction
    assert kept[(MR.OVER_MIN, (1, 2))] == 2  # at the default the eight neighbours are the two motions
    # dup: the exact copy goes where its original goes; the weak copy numbered below the strong ones folds INTO a higher number
    for m in (MR.OVER_MIN, MR.OVER_UNION):
        for f in FRACTIONS:
            rec, parent, x, count = _merged(pkg, O, "dup", measure=m, num=f[0], den=f[1])
            assert parent[5] == parent[1] != 5 and rec["count"][5] == rec["count"][1] == x[1, 5] >= 1
    rec, parent, x, count = _merged(pkg, O, "dup")
    assert parent[0] > 0 and rec["score"][parent[0]] > rec["score"][0] > 0  # by strength, not by number
    assert parent[6] == 6 and parent[7] == 7 and count.tolist() == [3, 8] and parent[3] == 3 and rec["count"][3] == 0  # (an empty valid pose stays)
    # nested: one support inside another; only containment folds at num == den
    rec, parent, x, count = _merged(pkg, O, "nested", num=1, den=1)
    assert 3 <= x[0, 2] == rec["count"][0] < rec["count"][2] and parent.tolist() == [2, 1, 2]
    # invalid poses are out and claim nothing; the hostile pose and the far one are valid and empty
    rec, parent, x, count = _merged(pkg, O, "invalid")
    assert rec["status"].tolist() == [SC_OK, SC_EINVAL, SC_OK, SC_OK, SC_OK, SC_ENOHYP] and parent.tolist() == [0, -1, 2, 3, 4, 0]
    assert rec["count"][[1, 2, 3]].tolist() == [0, 0, 0] and not x[1].any() and not x[:, 1].any() and count.tolist() == [4, 5]
    assert rec["Rt"][1].tobytes() == MR.IDENT.tobytes() == rec["Rt"][5].tobytes() and rec["Rt"][0].tobytes() == MR.lists(pkg)["invalid"][0].tobytes()
    # starved: a min_count that drops valid poses and keeps at least two
    rec, parent, x, count = _merged(pkg, O, "starved", min_count=7)
    dropped = (parent == -1) & (rec["status"] == SC_ENOHYP)
    assert dropped.sum() >= 1 and count[0] >= 2 and count[1] == 8 and (rec["count"][dropped] < 7).all() and rec["count"][dropped].max() >= 1
    assert (rec["index"] == parent).all()


def test_the_reference_keeps_the_headers_equalities(pkg, O):
    mo = MR.motions(pkg)
    S = MR.lists(pkg)
    n = len(mo.src)
    sel = (np.arange(n) % 3 != 0).astype(np.uint8)
    # (1) the score is sc_polish_poses's score0 under the same selection, in all three score modes
    for name in ("dup", "near", "invalid"):
        for score_mode in (0, 1, 2):
            for part, mode in ((None, PF.SEL_NONE), (sel, PF.SEL_MASK)):
                rec = MR.merge(O, mo.src, mo.tgt, S[name], MR.TAU, part=part, score_mode=score_mode)[0]
                pol = PF.poses(O, mo.src, mo.tgt, S[name], MR.TAU, mode, part, score_mode=score_mode, max_iter=1)[0]
                assert np.array_equal(rec["score"], pol["score0"]), (name, score_mode)
                masks = [(O.mask(mo.src, mo.tgt, p, MR.TAU) != 0) & (True if part is None else part != 0) if np.isfinite(p).all() else np.zeros(n, bool)
                         for p in S[name]]
                assert rec["count"].tolist() == [int(m.sum()) for m in masks]
    # (2) an exact copy goes where its lowest-numbered original goes, for every fraction and either measure (also num == den == 65536)
    for m in (MR.OVER_MIN, MR.OVER_UNION):
        for num, den in FRACTIONS + ((65536, 65536), (1, 65536)):
            parent = MR.merge(O, mo.src, mo.tgt, S["many64"], MR.TAU, measure=m, num=num, den=den)[1]
            assert parent[5] == parent[1] != 5
    # (3) the kept records go in again and are all kept, byte for byte
    for name in ("dup", "near", "starved", "invalid"):
        for compact in (False, True):
            rec, parent, x, count = MR.merge(O, mo.src, mo.tgt, S[name], MR.TAU, compact=compact)
            again = MR.merge(O, mo.src, mo.tgt, rec["Rt"], MR.TAU, statuses=rec["status"], compact=compact)
            kept = rec["status"] == SC_OK
            assert again[3][0] == count[0] == kept.sum() and again[0]["Rt"][kept].tobytes() == rec["Rt"][kept].tobytes()
            assert np.array_equal(again[0]["status"], rec["status"]) and np.array_equal(again[0]["count"][kept], rec["count"][kept])
            if compact:
                assert kept[:count[0]].all() and not kept[count[0]:].any() and (np.diff(rec["index"][:count[0]]) > 0).all()
    # (5) num == den under OVER_MIN: folded exactly when one support holds the other
    for name in ("dup", "near", "nested", "starved"):
        rec, parent, x, count = MR.merge(O, mo.src, mo.tgt, S[name], MR.TAU, num=3, den=3)
        keptk = [k for k in range(len(parent)) if parent[k] == k]
        for k in range(len(parent)):
            if parent[k] < 0 or parent[k] == k:
                continue
            j = parent[k]
            assert x[j, k] == min(x[j, j], x[k, k]) >= 1
        for k in keptk:  # ... and a kept pose holds no stronger kept pose's support, nor is held by one
            for j in keptk:
                if j != k:
                    assert x[j, k] < min(x[j, j], x[k, k]) or x[j, k] == 0
    # the batch wrapper is the frame reference per problem; a problem with a NaN coordinate is SC_EINVAL throughout
    two = S["near"][[0, 4, 5]]
    bad = mo.src[700:900].copy(); bad[7, 1] = np.nan
    out, parent, count = MR.batch(O, [(mo.src[:300], mo.tgt[:300]), (bad, mo.tgt[700:900]), (mo.src[300:700], mo.tgt[300:700])],
                                  np.stack([two, two, two], axis=1), MR.TAU)
    one = MR.merge(O, mo.src[300:700], mo.tgt[300:700], two, MR.TAU, statuses=np.zeros(3, np.int32))
    assert out[:, 2].tobytes() == one[0].tobytes() and np.array_equal(parent[:, 2], one[1]) and count[2].tolist() == one[3].tolist()
    assert (out[:, 1]["status"] == SC_EINVAL).all() and (parent[:, 1] == -1).all() and count[1].tolist() == [0, 0] and not out[:, 1]["count"].any()
