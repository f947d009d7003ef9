"""CPU suite: the surface of sc_settle_poses (include/saccot.h) — the five exports, the Python mirror, the layout of sc_settle_params,
the default parameters, the macros, the argument checks that need no GPU (also under the sanitizers, in a program of their own) — and
the Python restatement of its semantics (tests/settle_ref.py) that the GPU tests compare against: its pose lists are checked for
what they are used for, and the equalities the header promises hold on the references themselves.  No compute call reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import polish_poses_ref as PF
import settle_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_settle_default_params", "sc_settle_poses_frame", "sc_settle_poses_frame_device", "sc_settle_poses_batch",
         "sc_settle_poses_batch_device")
SC_OK, SC_EINVAL = 0, -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_settle_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    for method in ("settle_poses_frame", "settle_poses_frame_device", "settle_poses_batch", "settle_poses_batch_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.ScSettleParams is pkg.api.ScSettleParams and callable(pkg.make_settle_params)
    assert (pkg.SC_SETTLE_MAX_POSES, pkg.SC_SETTLE_BATCH_MAX_POSES, pkg.SC_SETTLE_STATUS) == (64, 16, 1)
    assert pkg.SC_SETTLE_BATCH_MAX_POSES == pkg.api.SC_INSTANCES_BATCH_MAX  # a plane of sc_register_instances_batch per pose
    block = header[header.index("sc_settle_poses ---"):]
    for word in ("merging or dropping poses", "soft assignment", "slots and pairs forms", "sharded frames"):
        assert word in block  # what is not here is said
    assert "sc_settle_poses, below" in header  # sc_assign_poses's "Not here" points at this entry


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_SETTLE 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_the_struct_layout_and_the_macros_in_c(pkg, tmp_path):
    exe = str(tmp_path / "settle_layout")
    P = "sc_settle_params"
    fields = [f"sizeof({P})"] + [f"offsetof({P}, {f})" for f in ("size", "max_iter", "sel_mode", "flags", "reserved")]
    consts = ["SC_SETTLE_MAX_POSES", "SC_SETTLE_BATCH_MAX_POSES", "SC_SETTLE_STATUS", "SC_HAS_SETTLE", "SC_INSTANCES_BATCH_MAX"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("' + "%zu " * len(fields) + "%u " * len(consts)
           + '", ' + ", ".join(fields) + ", " + ", ".join(f"(unsigned){c}" for c in consts) + ");return 0;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    K = pkg.api.ScSettleParams
    assert got[:6] == [32, 0, 4, 8, 12, 16]
    assert got[:6] == [C.sizeof(K), K.size.offset, K.max_iter.offset, K.sel_mode.offset, K.flags.offset, K.reserved.offset]
    assert got[6:] == [64, 16, 1, 1, 16]


def test_default_params_and_null_arguments(pkg):
    L = pkg.load_library()
    sp = pkg.ScSettleParams()
    sp.reserved[2] = 9
    assert L.sc_settle_default_params(C.byref(sp)) == SC_OK
    assert (sp.size, sp.max_iter, sp.sel_mode, sp.flags, list(sp.reserved)) == (32, 16, 0, 0, [0, 0, 0, 0])
    assert L.sc_settle_default_params(None) == SC_EINVAL
    mk = pkg.make_settle_params(max_iter=3, sel_mode=1, flags=1)
    assert (mk.size, mk.max_iter, mk.sel_mode, mk.flags) == (32, 3, 1, 1)
    # a NULL context is refused before anything is touched, in all four entries
    assert L.sc_settle_poses_frame(None, C.byref(sp), None, 48, 1, None, None, None, None, None) == SC_EINVAL
    assert L.sc_settle_poses_frame_device(None, C.byref(sp), None, 48, 1, None, None, None, None, None) == SC_EINVAL
    assert L.sc_settle_poses_batch(None, None, None, None, 0, None, None, None, 0, 0, None, None, None) == SC_EINVAL
    assert L.sc_settle_poses_batch_device(None, None, None, None, 0, None, None, None, 0, 0, None, None, None) == SC_EINVAL


def test_the_host_checks_under_the_sanitizers(tmp_path):
    """Every refusal rule of sc_settle_check.hpp and the bytes read of the pose array: tests/native/settle_check_main.cpp, a program
    of its own built with -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "settle_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "settle_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


# ---- the reference itself: the pose lists are what they are used for ---------------------------------------------------------------
def _settled(pkg, O, name, **kw):
    mo = SR.motions(pkg)
    out = SR.settle(O, mo.src, mo.tgt, SR.starts(pkg)[name], SR.TAU, **kw)
    print(name, kw, "rounds", out[3].tolist(), "iters", out[0]["iters"].tolist(), "stops", out[0]["stop"].tolist(), "scores", out[0]["score"].tolist())
    return mo, out


def test_the_pose_lists_settle_as_the_gpu_tests_need_them_to(pkg, O):
    for name in ("gt", "perturbed"):
        mo, (rec, lab, d2, rounds) = _settled(pkg, O, name)
        assert rounds[1] == SR.STOP_FIXED and rounds[0] >= 2 and (rec["stop"] == SR.STOP_FIXED).all() and (rec["status"] == SC_OK).all()
        assert 1 <= rec["iters"].max() <= rounds[0]  # a pose moves in counted rounds only
        for k in range(2):  # each pose ends on its own motion: most of its true correspondences carry its label
            assert ((lab == k) & (mo.label == k)).sum() > 0.9 * (mo.label == k).sum()
        assert np.array_equal(rec["score"], np.bincount(lab[lab >= 0], minlength=2))  # the inlier-count mode: the tally is the label's size
    mo, (rec, lab, d2, rounds) = _settled(pkg, O, "far_dup")
    assert rounds[1] == SR.STOP_FIXED and rounds[0] >= 2
    assert rec["stop"].tolist()[2] == SR.STOP_DECLINED and rec["iters"][2] == 0 and rec["score"][2] == 0  # the far pose claims nothing
    assert (rec["stop"][[0, 1, 3]] == SR.STOP_FIXED).all() and rec["score"][3] > 0  # the copy and its original split the inliers: no merging
    assert rec["Rt"][2].tobytes() == SR.starts(pkg)["far_dup"][2].tobytes()
    mo, (rec, lab, d2, rounds) = _settled(pkg, O, "many8")
    assert rounds.tolist() == [16, SR.STOP_MAX_ITER] and (rec["stop"] == SR.STOP_MAX_ITER).sum() >= 4 and rec["iters"].max() == 16
    mo, (rec, lab, d2, rounds) = _settled(pkg, O, "many64", max_iter=2)
    assert rounds.tolist() == [2, SR.STOP_MAX_ITER]
    assert (rec["stop"] == SR.STOP_DECLINED).sum() >= 8 and (rec["stop"] == SR.STOP_MAX_ITER).sum() >= 8  # starved poses beside live ones
    assert ((rec["stop"] == SR.STOP_DECLINED) & (rec["score"] > 0) & (rec["score"] < 3)).any()  # ... some with fewer than 3 members


def test_the_reference_keeps_the_headers_equalities(pkg, O):
    mo = SR.motions(pkg)
    S = SR.starts(pkg)
    # (1) the composed loop
    for name, max_iter in (("perturbed", 16), ("far_dup", 16), ("many8", 2)):
        rec, lab, d2, rounds = SR.settle(O, mo.src, mo.tgt, S[name], SR.TAU, max_iter=max_iter)
        R = int(rounds[0]) + (1 if rounds[1] == SR.STOP_FIXED else 0)
        Rt, clab, cd2, casg = SR.composed(O, mo.src, mo.tgt, S[name], SR.TAU, R)
        assert Rt.tobytes() == rec["Rt"].tobytes() and np.array_equal(clab, lab) and cd2.tobytes() == d2.tobytes(), name
        assert np.array_equal(casg["score"], rec["score"]), name
    # (2) one pose: sc_polish_poses's record, and the label is its mask
    for max_iter in (1, 2, 16):
        rec, lab, d2, rounds = SR.settle(O, mo.src, mo.tgt, S["perturbed"][:1], SR.TAU, max_iter=max_iter)
        pol, mask = PF.poses(O, mo.src, mo.tgt, S["perturbed"][:1], SR.TAU, max_iter=max_iter)
        assert rec.tobytes() == pol.tobytes() and np.array_equal(lab, mask[0].astype(np.int32) - 1), max_iter
    # (4) a settled list goes in again
    rec, lab, d2, rounds = SR.settle(O, mo.src, mo.tgt, S["far_dup"], SR.TAU)
    again = SR.settle(O, mo.src, mo.tgt, rec["Rt"], SR.TAU, statuses=rec["status"])
    assert again[3].tolist() == [0, SR.STOP_FIXED] and again[0]["Rt"].tobytes() == rec["Rt"].tobytes() and np.array_equal(again[1], lab)
    assert not again[0]["iters"].any() and np.array_equal(again[0]["score"], rec["score"]) and np.array_equal(again[0]["score0"], rec["score"])
    # invalid poses: the status passed through, a non-finite Rt, both with sc_polish_poses's record; they change nothing else
    poses = np.concatenate([S["perturbed"], S["perturbed"]])
    poses[3][5] = np.nan
    st = np.array([0, 0, SR.SC_ENOHYP, 0], np.int32)
    rec, lab, d2, rounds = SR.settle(O, mo.src, mo.tgt, poses, SR.TAU, statuses=st)
    good = SR.settle(O, mo.src, mo.tgt, S["perturbed"], SR.TAU)
    assert rec["status"].tolist() == [0, 0, SR.SC_ENOHYP, SC_EINVAL] and rec[:2].tobytes() == good[0].tobytes() and np.array_equal(lab, good[1])
    assert rec["Rt"][2].tobytes() == SR.IDENT.tobytes() and rec["stop"][2:].tolist() == [SR.STOP_DECLINED] * 2 and not rec["score"][2:].any()
    # the batch wrapper is the frame reference per problem
    out, labels, rr = SR.batch(O, [(mo.src[:300], mo.tgt[:300]), (mo.src[300:700], mo.tgt[300:700])],
                               np.stack([S["perturbed"], S["perturbed"]], axis=1), SR.TAU)
    one = SR.settle(O, mo.src[300:700], mo.tgt[300:700], S["perturbed"], SR.TAU, statuses=np.zeros(2, np.int32))
    assert out[:, 1].tobytes() == one[0].tobytes() and np.array_equal(labels[1], one[1]) and rr[1].tolist() == one[3].tolist()
