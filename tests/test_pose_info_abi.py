"""CPU suite: the surface of sc_pose_info_batch (include/saccot.h) — the four exports, the Python mirror, the struct layout, the
argument checks that need no GPU — and the Python restatement of its semantics (tests/pose_info_ref.py) that the GPU tests compare
against, checked here for what its scenes are used for and for the sign convention and the assembly of the matrix.  No compute call
reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import pose_info_ref as PI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_pose_info_batch", "sc_pose_info_batch_device", "sc_pose_info_batch_slots_device", "sc_pose_info_pairs_slots_device")
SC_OK, SC_EINVAL = 0, -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_pose_info_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("pose_info_batch_raw", "pose_info_batch_device", "pose_info_batch_slots_device", "pose_info_pairs_slots_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.ScPoseInfoResult is pkg.api.ScPoseInfoResult and pkg.POSE_INFO_RESULT_DTYPE is pkg.api.POSE_INFO_RESULT_DTYPE


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_POSE_INFO 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_pose_info_result_layout(pkg):
    exe = os.path.join(ROOT, "tests", ".abi_probe_pose_info")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d", '
           'sizeof(sc_pose_info_result), offsetof(sc_pose_info_result, info), offsetof(sc_pose_info_result, sse), '
           'offsetof(sc_pose_info_result, status), offsetof(sc_pose_info_result, inliers), offsetof(sc_pose_info_result, reserved), '
           'sizeof(sc_batch_result), sizeof(sc_polish_batch_result), SC_HAS_POSE_INFO);return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    finally:
        os.remove(exe)
    K = pkg.api.ScPoseInfoResult
    assert got[:6] == [320, 0, 288, 296, 300, 304]
    assert got[:6] == [C.sizeof(K), K.info.offset, K.sse.offset, K.status.offset, K.inliers.offset, K.reserved.offset]
    assert got[6:8] == [80, 64] == [C.sizeof(pkg.ScBatchResult), C.sizeof(pkg.ScPolishBatchResult)]  # the existing records did not move
    assert got[8] == 1
    for dt in (pkg.api.POSE_INFO_RESULT_DTYPE, PI.RESULT_DTYPE):
        assert dt.itemsize == 320 and [dt.fields[k][1] for k in ("info", "sse", "status", "inliers", "reserved")] == [0, 288, 296, 300, 304]
    # both pose-carrying records hold Rt at byte 0 and status at byte 48
    for dt in (pkg.BATCH_RESULT_DTYPE, pkg.api.POLISH_BATCH_RESULT_DTYPE):
        assert (dt.fields["Rt"][1], dt.fields["status"][1]) == (0, 48)


def test_null_arguments_and_bad_strides_are_refused_without_a_gpu(pkg):
    L = pkg.load_library()
    p = pkg.make_params(**PI.kw_of(0.02))
    off = np.array([0, 8], np.uint32)
    o = off.ctypes.data_as(C.POINTER(C.c_uint32))
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on the NULL context before it looks at anything else
    f32 = np.zeros((8, 3), np.float32).ctypes.data_as(C.POINTER(C.c_float))
    # (a context cannot exist here — sc_create fails without a GPU — so the NULL arguments and the bad strides are tried with a NULL
    # context; the GPU suite repeats them on a real one, where sc_last_error names the reason)
    for stride in (80, 64, 0, 50, 54):
        assert L.sc_pose_info_batch(None, f32, f32, o, 1, C.byref(p), fake, stride, fake) == SC_EINVAL
        assert L.sc_pose_info_batch_device(None, fake, fake, o, 1, C.byref(p), fake, stride, fake) == SC_EINVAL
        assert L.sc_pose_info_batch_slots_device(None, fake, o, fake, o, 1, 1, C.byref(p), fake, fake, fake, stride, fake) == SC_EINVAL
        assert L.sc_pose_info_pairs_slots_device(None, fake, o, 1, o, 1, 1, C.byref(p), fake, fake, fake, stride, fake) == SC_EINVAL
    assert L.sc_pose_info_batch(None, None, f32, o, 1, C.byref(p), fake, 80, fake) == SC_EINVAL
    assert L.sc_pose_info_batch(None, f32, f32, o, 1, None, None, 80, None) == SC_EINVAL
    assert L.sc_pose_info_batch_device(None, fake, fake, None, 1, C.byref(p), None, 80, None) == SC_EINVAL
    assert L.sc_pose_info_batch_slots_device(None, None, o, fake, None, 1, 1, None, fake, fake, None, 80, fake) == SC_EINVAL
    assert L.sc_pose_info_pairs_slots_device(None, None, None, 1, None, 1, 1, None, fake, fake, None, 80, fake) == SC_EINVAL


# ---- the scenes are what the GPU tests use them for, and the matrix is sum J^T J: asserted on the reference alone -------------
def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def _check_against_numpy(O, src, tgt, Rt, tau, rec):
    """info == sum J^T J, J = [-[x]x | I], built by numpy from the reference's own x: entrywise within (n + 3) 2^-52 sum |J|^T |J|,
    which bounds the summation error of n rounded adds (the products and the one add of an entry's assembly take the other 3) — only
    the sign convention and the assembly are under test here.  The matrix is symmetric bit for bit and its translation block is c I."""
    mask, x, e = PI.terms(O, src, tgt, Rt, tau)
    n, c = len(src), int(mask.sum())
    assert int(rec["inliers"]) == c and int(rec["status"]) == SC_OK
    want = np.zeros((6, 6)); bound = np.zeros((6, 6))
    for m in np.flatnonzero(mask):
        J = np.hstack([-_skew(x[m]), np.eye(3)])
        want += J.T @ J
        bound += np.abs(J).T @ np.abs(J)
    info = rec["info"].reshape(6, 6)
    assert (np.abs(info - want) <= (n + 3) * 2.0 ** -52 * bound).all()
    assert info.tobytes() == np.ascontiguousarray(info.T).tobytes()
    assert float(rec["info"][21]) == float(rec["info"][28]) == float(rec["info"][35]) == float(c)
    sse = float(sum(float(e[m] @ e[m]) for m in np.flatnonzero(mask)))
    assert abs(float(rec["sse"]) - sse) <= (n + 3) * 2.0 ** -52 * sse
    return mask


def test_the_crafted_scenes_are_what_they_are_used_for(O):
    names, problems, poses = PI.crafted()
    assert names == ("last", "hole", "none", "two", "huge")
    assert [len(s) for s, _ in problems] == [129, 192, 64, 65, 70]
    recs = PI.batch(O, problems, poses, 0.05)
    masks = {}
    for b, name in enumerate(names):
        s, t = problems[b]
        if name == "huge":  # (numpy's float64 products of such x overflow nothing either: 9e76 x 70)
            assert np.abs(s).max() == PI.FLT_BIG and np.array_equal(s, t)
        masks[name] = _check_against_numpy(O, s, t, poses[b]["Rt"], 0.05, recs[b])
    print({k: int(v.sum()) for k, v in masks.items()})
    assert np.flatnonzero(masks["last"]).tolist() == [128]                        # every inlier in the last chunk; c == 1
    hole = masks["hole"]
    assert hole[:64].any() and not hole[64:128].any() and hole[128:].any()        # an empty middle chunk
    assert not masks["none"].any()                                                 # c == 0 ...
    assert recs[2].tobytes() == bytes(320)                                         # ... is SC_OK with all zeros
    assert np.flatnonzero(masks["two"]).tolist() == [63, 64]                       # c == 2, one either side of a chunk end
    assert masks["huge"].all() and float(recs[4]["sse"]) == 0.0 and np.isfinite(recs[4]["info"]).all()
    assert float(np.abs(recs[4]["info"]).max()) > 1e77                             # products near FLT_MAX^2 were summed
    assert [int(r["inliers"]) for r in recs] == [1, int(hole.sum()), 0, 2, 70]


def test_the_mixed_scene_at_a_ground_truth_like_pose(pkg, O):
    """the sizes of the mixed batch, each at its scene's true pose rounded to fp32: inliers in every chunk, up to eight chunks"""
    assert [len(s) for s, _ in PI.mixed(pkg)] == [3, 4, 63, 64, 65, 128, 129, 257, 512, 512]
    many = 0
    for n, rho in ((65, .3), (129, .3), (257, .25), (512, .3)):
        sc = pkg.synth.make_scene(n, rho, 1.0, 0.05, 7000 + n)  # batch_ref.scene's
        Rt = np.concatenate([np.asarray(sc.R_gt, np.float32).ravel(), np.asarray(sc.t_gt, np.float32).ravel()])
        rec = PI.one(O, sc.src, sc.tgt, SC_OK, Rt, 0.05)
        mask = _check_against_numpy(O, sc.src, sc.tgt, Rt, 0.05, rec)
        chunks = [bool(mask[lo: lo + 64].any()) for lo in range(0, n, 64)]
        print(n, int(mask.sum()), chunks)
        many += int(mask.sum()) >= 0.2 * n and sum(chunks) >= 2
    assert many >= 3


def test_status_rules_of_the_reference(O):
    _, problems, poses = PI.crafted()
    s, t = problems[1]
    Rt = poses[1]["Rt"]
    nan_t = t.copy(); nan_t[5, 1] = np.nan
    bad_rt = Rt.copy(); bad_rt[7] = np.nan
    for (a, b, st, rt), want in (((s, nan_t, SC_OK, Rt), SC_EINVAL), ((s, t, SC_OK, bad_rt), SC_EINVAL), ((s, t, PI.SC_ENOHYP, Rt), PI.SC_ENOHYP)):
        out = PI.one(O, a, b, st, rt, 0.05)
        zero = np.zeros((), PI.RESULT_DTYPE); zero["status"] = want
        assert out.tobytes() == zero.tobytes()
    # the slot form: flagged, short, an index outside the problem
    corr = np.stack([np.arange(len(s)), np.arange(len(s))], 1).astype(np.int32)
    full = PI.one(O, s, t, SC_OK, Rt, 0.05)
    assert PI.slots_one(O, s, t, corr, len(s), 0, SC_OK, Rt, 0.05).tobytes() == full.tobytes()
    assert int(PI.slots_one(O, s, t, corr, len(s), 1, SC_OK, Rt, 0.05)["status"]) == SC_EINVAL
    assert int(PI.slots_one(O, s, t, corr, 2, 0, PI.SC_ENOHYP, Rt, 0.05)["status"]) == PI.SC_ENOHYP
    assert int(PI.slots_one(O, s, t, corr, 2, 0, SC_OK, Rt, 0.05)["status"]) == SC_EINVAL
    out_of = corr.copy(); out_of[9, 1] = len(t)
    assert int(PI.slots_one(O, s, t, out_of, len(s), 0, SC_OK, Rt, 0.05)["status"]) == SC_EINVAL
