"""CPU suite: the surface of sc_pose_info_frame (include/saccot.h) — the three exports, the Python mirror, the layout of
sc_pose_info_params, the default parameters, the argument checks that need no GPU — and the Python restatement of its semantics
(tests/pose_info_frame_ref.py) that the GPU tests compare against, checked here for what its scenes are used for.  No compute call
reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import pose_info_frame_ref as PF
import pose_info_ref as PI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_pose_info_default_params", "sc_pose_info_frame", "sc_pose_info_frame_device")
SC_OK, SC_EINVAL = 0, -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_pose_info_frame_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("pose_info_frame", "pose_info_frame_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.ScPoseInfoParams is pkg.api.ScPoseInfoParams and callable(pkg.make_pose_info_params)
    assert (pkg.SC_POSE_INFO_SEL_NONE, pkg.SC_POSE_INFO_SEL_MASK, pkg.SC_POSE_INFO_SEL_LABEL, pkg.SC_POSE_INFO_STATUS,
            pkg.SC_POSE_INFO_MAX_POSES) == (0, 1, 2, 1, 1024)


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_POSE_INFO_FRAME 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_pose_info_params_layout_and_constants(pkg):
    exe = os.path.join(ROOT, "tests", ".abi_probe_pose_info_frame")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %u %u %u %u %u %d", '
           'sizeof(sc_pose_info_params), offsetof(sc_pose_info_params, size), offsetof(sc_pose_info_params, sel_mode), '
           'offsetof(sc_pose_info_params, label0), offsetof(sc_pose_info_params, flags), offsetof(sc_pose_info_params, reserved), '
           'sizeof(sc_pose_info_result), SC_POSE_INFO_SEL_NONE, SC_POSE_INFO_SEL_MASK, SC_POSE_INFO_SEL_LABEL, SC_POSE_INFO_STATUS, '
           'SC_POSE_INFO_MAX_POSES, SC_HAS_POSE_INFO_FRAME);return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    finally:
        os.remove(exe)
    K = pkg.api.ScPoseInfoParams
    assert got[:6] == [32, 0, 4, 8, 12, 16]
    assert got[:6] == [C.sizeof(K), K.size.offset, K.sel_mode.offset, K.label0.offset, K.flags.offset, K.reserved.offset]
    assert got[6] == 320 == C.sizeof(pkg.ScPoseInfoResult)  # the record is the batch form's, and did not move
    assert got[7:] == [0, 1, 2, 1, 1024, 1]
    # the pose sources of the contract: Rt at byte 0 in each; a status at byte 48 where the flag applies, the rank of a polish candidate
    for dt, stride, word in ((pkg.BATCH_RESULT_DTYPE, 80, "status"), (pkg.api.POLISH_BATCH_RESULT_DTYPE, 64, "status"),
                             (pkg.api.POLISH_CAND_DTYPE, 64, "rank")):
        assert dt.itemsize == stride and (dt.fields["Rt"][1], dt.fields[word][1]) == (0, 48)


def test_default_params(pkg):
    L = pkg.load_library()
    ip = pkg.ScPoseInfoParams(1, 2, 3, 4)
    ip.reserved[2] = 9
    assert L.sc_pose_info_default_params(C.byref(ip)) == SC_OK
    assert bytes(ip) == (32).to_bytes(4, "little") + bytes(28)
    assert L.sc_pose_info_default_params(None) == SC_EINVAL
    assert bytes(pkg.make_pose_info_params()) == bytes(ip)
    q = pkg.make_pose_info_params(sel_mode=pkg.SC_POSE_INFO_SEL_LABEL, label0=-3, flags=pkg.SC_POSE_INFO_STATUS)
    assert (q.size, q.sel_mode, q.label0, q.flags, list(q.reserved)) == (32, 2, -3, 1, [0, 0, 0, 0])


def test_every_argument_is_refused_without_a_context(pkg):
    L = pkg.load_library()
    ip = pkg.make_pose_info_params()
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on the NULL context before it looks at anything else
    # (a context cannot exist here — sc_create fails without a GPU —; the GPU suite repeats every rule on a real one, where
    # sc_last_error names the reason)
    for entry in (L.sc_pose_info_frame, L.sc_pose_info_frame_device):
        for stride in (48, 64, 80, 0, 44, 50):
            for n_poses in (1, 0, 1025):
                assert entry(None, C.byref(ip), fake, stride, n_poses, None, fake) == SC_EINVAL
        assert entry(None, None, fake, 48, 1, None, fake) == SC_EINVAL
        assert entry(None, C.byref(ip), None, 48, 1, None, fake) == SC_EINVAL
        assert entry(None, C.byref(ip), fake, 48, 1, None, None) == SC_EINVAL
        for bad in (pkg.ScPoseInfoParams(31, 0, 0, 0), pkg.make_pose_info_params(sel_mode=3), pkg.make_pose_info_params(sel_mode=1),
                    pkg.make_pose_info_params(label0=1), pkg.make_pose_info_params(flags=2)):
            assert entry(None, C.byref(bad), fake, 64, 1, None, fake) == SC_EINVAL


# ---- the scenes are what the GPU tests use them for: asserted on the reference alone ---------------------------------------------
def test_the_large_scene_needs_more_than_one_round_of_the_deal(pkg, O):
    assert PF.SIZES == (65, 129, 512, 6600)
    nch = (max(PF.SIZES) + 63) // 64
    assert nch > 102 and 10 * nch > 1024  # the chains of one pose exceed one round of 1024 lanes
    for n in PF.SIZES[:3]:  # every chunk layout at a ground-truth-like pose: inliers in every chunk
        sc = PF.scene(pkg, n)
        Rt = PF.rt_of(sc.R_gt, sc.t_gt)
        rec = PF.one(O, sc.src, sc.tgt, Rt, PF.TAU)
        mask = PI.terms(O, sc.src, sc.tgt, Rt, PF.TAU)[0]
        print(n, int(rec["inliers"]))
        assert int(rec["status"]) == SC_OK and int(rec["inliers"]) == int(mask.sum()) >= 0.2 * n
        assert all(mask[lo: lo + 64].any() for lo in range(0, n - n % 64, 64))
        # no selection: the frame form IS the batch form
        assert rec.tobytes() == PI.one(O, sc.src, sc.tgt, SC_OK, Rt, PF.TAU).tobytes()


def test_the_mask_scenes_deselect_inliers(O):
    src, tgt, Rt, sel = PF.crafted_hole()
    mask = PI.terms(O, src, tgt, Rt, PF.TAU)[0].astype(bool)
    assert len(src) == 192 and not sel[64:128].any() and sel[:64].all() and sel[128:].all()  # one whole interior chunk is deselected ...
    assert mask[64:128].sum() >= 3                                                             # ... and holds inliers of the pose
    assert mask[:64].any() and mask[128:].any()
    full, holed = PF.one(O, src, tgt, Rt, PF.TAU), PF.frame(O, src, tgt, [Rt], PF.TAU, PF.SEL_MASK, sel)[0]
    assert int(holed["inliers"]) == int((mask & (sel != 0)).sum()) == int(full["inliers"]) - int(mask[64:128].sum())
    assert holed.tobytes() != full.tobytes()  # a kernel that ignored sel could not pass
    # a chunk without a set bit adds 0.0, which changes no sum: the record is that of the two outer chunks alone
    outer = np.r_[0:64, 128:192]
    alone = PF.one(O, src[outer], tgt[outer], Rt, PF.TAU)
    assert holed.tobytes() == alone.tobytes()
    src, tgt, Rt, sel = PF.crafted_last()
    mask = PI.terms(O, src, tgt, Rt, PF.TAU)[0].astype(bool)
    assert len(src) == 129 and np.flatnonzero(sel).tolist() == [128] and mask[128] and mask[:128].sum() >= 3
    rec = PF.frame(O, src, tgt, [Rt], PF.TAU, PF.SEL_MASK, sel)[0]
    assert int(rec["inliers"]) == 1 and int(rec["status"]) == SC_OK and float(rec["info"][21]) == 1.0


def test_the_label_scene_and_the_far_pose(pkg, O):
    sc = PF.motions(pkg)
    poses = [PF.rt_of(R, t) for R, t in sc.motions]
    assert len(poses) == 2 and len(sc.src) == 1500
    recs = PF.frame(O, sc.src, sc.tgt, poses, PF.TAU, PF.SEL_LABEL, sc.label)
    print([int(r["inliers"]) for r in recs])
    assert all(int(r["inliers"]) >= 3 for r in recs)  # two labels each own at least 3 inliers
    shifted = PF.frame(O, sc.src, sc.tgt, poses, PF.TAU, PF.SEL_LABEL, sc.label + 7, label0=7)
    assert shifted.tobytes() == recs.tobytes()
    wrong = PF.frame(O, sc.src, sc.tgt, poses, PF.TAU, PF.SEL_LABEL, sc.label, label0=1)
    assert int(wrong[0]["inliers"]) < int(recs[0]["inliers"])  # pose 0 on motion 1's correspondences
    for Rt in poses:
        rec = PF.one(O, sc.src, sc.tgt, PF.far(Rt), PF.TAU)
        assert rec.tobytes() == bytes(320)  # the far-away pose: 0 inliers, SC_OK, all zeros


def test_status_rules_of_the_reference(pkg, O):
    sc = PF.scene(pkg, 129)
    Rt = PF.rt_of(sc.R_gt, sc.t_gt)
    good = PF.one(O, sc.src, sc.tgt, Rt, PF.TAU)
    bad = Rt.copy(); bad[4] = np.inf
    zero = np.zeros((), PF.RESULT_DTYPE)
    got = PF.frame(O, sc.src, sc.tgt, [Rt, Rt, bad, Rt], PF.TAU, statuses=[SC_OK, PF.SC_ENOHYP, SC_OK, 77])
    zero["status"] = PF.SC_ENOHYP
    assert got[0].tobytes() == good.tobytes() and got[1].tobytes() == zero.tobytes()
    zero["status"] = SC_EINVAL
    assert got[2].tobytes() == zero.tobytes()
    zero["status"] = 77
    assert got[3].tobytes() == zero.tobytes()
    # without the flag the word at byte 48 is not a status
    assert PF.frame(O, sc.src, sc.tgt, [Rt], PF.TAU)[0].tobytes() == good.tobytes()
