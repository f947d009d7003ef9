"""CPU suite: the surface of sc_polish_poses (include/saccot.h) — the three exports, the Python mirror, the layout of
sc_polish_poses_params, the default parameters, the argument checks that need no GPU — and the Python restatement of its semantics
(tests/polish_poses_ref.py) that the GPU tests compare against, checked here for what its scenes are used for.  No compute call
reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import polish_poses_ref as PF
import polish_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_polish_poses_default_params", "sc_polish_poses", "sc_polish_poses_device")
SC_OK, SC_EINVAL = 0, -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_polish_poses_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("polish_poses", "polish_poses_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.ScPolishPosesParams is pkg.api.ScPolishPosesParams and callable(pkg.make_polish_poses_params)
    assert (pkg.SC_POLISH_POSES_SEL_NONE, pkg.SC_POLISH_POSES_SEL_MASK, pkg.SC_POLISH_POSES_SEL_LABEL, pkg.SC_POLISH_POSES_SEL_ALIVE,
            pkg.SC_POLISH_POSES_STATUS, pkg.SC_POLISH_POSES_MAX) == (0, 1, 2, 3, 1, 1024)


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_POLISH_POSES 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_polish_poses_params_layout_and_constants(pkg):
    exe = os.path.join(ROOT, "tests", ".abi_probe_polish_poses")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %u %u %u %u %u %u %d", '
           'sizeof(sc_polish_poses_params), offsetof(sc_polish_poses_params, size), offsetof(sc_polish_poses_params, max_iter), '
           'offsetof(sc_polish_poses_params, sel_mode), offsetof(sc_polish_poses_params, label0), offsetof(sc_polish_poses_params, flags), '
           'offsetof(sc_polish_poses_params, reserved), sizeof(sc_polish_batch_result), SC_POLISH_POSES_SEL_NONE, SC_POLISH_POSES_SEL_MASK, '
           'SC_POLISH_POSES_SEL_LABEL, SC_POLISH_POSES_SEL_ALIVE, SC_POLISH_POSES_STATUS, SC_POLISH_POSES_MAX, SC_HAS_POLISH_POSES);return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    finally:
        os.remove(exe)
    K = pkg.api.ScPolishPosesParams
    assert got[:7] == [32, 0, 4, 8, 12, 16, 20]
    assert got[:7] == [C.sizeof(K), K.size.offset, K.max_iter.offset, K.sel_mode.offset, K.label0.offset, K.flags.offset, K.reserved.offset]
    assert got[7] == 64 == C.sizeof(pkg.ScPolishBatchResult) == PF.RESULT_DTYPE.itemsize  # the record is the batch form's, and did not move
    assert got[8:] == [0, 1, 2, 3, 1, 1024, 1]
    # the output record is a pose record: Rt at byte 0, the status at byte 48
    dt = pkg.api.POLISH_BATCH_RESULT_DTYPE
    assert dt.itemsize == 64 and (dt.fields["Rt"][1], dt.fields["status"][1]) == (0, 48)


def test_default_params(pkg):
    L = pkg.load_library()
    qp = pkg.ScPolishPosesParams(1, 2, 3, 4, 5)
    qp.reserved[2] = 9
    assert L.sc_polish_poses_default_params(C.byref(qp)) == SC_OK
    assert bytes(qp) == (32).to_bytes(4, "little") + (16).to_bytes(4, "little") + bytes(24)
    assert L.sc_polish_poses_default_params(None) == SC_EINVAL
    assert bytes(pkg.make_polish_poses_params()) == bytes(qp)
    q = pkg.make_polish_poses_params(max_iter=3, sel_mode=pkg.SC_POLISH_POSES_SEL_ALIVE, label0=-3, flags=pkg.SC_POLISH_POSES_STATUS)
    assert (q.size, q.max_iter, q.sel_mode, q.label0, q.flags, list(q.reserved)) == (32, 3, 3, -3, 1, [0, 0, 0])


def test_every_argument_is_refused_without_a_context(pkg):
    L = pkg.load_library()
    qp = pkg.make_polish_poses_params()
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on the NULL context before it looks at anything else
    # (a context cannot exist here — sc_create fails without a GPU —; the GPU suite repeats every rule on a real one, where
    # sc_last_error names the reason)
    for entry in (L.sc_polish_poses, L.sc_polish_poses_device):
        for stride in (48, 64, 80, 0, 44, 50):
            for n_poses in (1, 0, 1025):
                for mask in (None, fake):
                    assert entry(None, C.byref(qp), fake, stride, n_poses, None, fake, mask) == SC_EINVAL
        assert entry(None, None, fake, 48, 1, None, fake, None) == SC_EINVAL
        assert entry(None, C.byref(qp), None, 48, 1, None, fake, None) == SC_EINVAL
        assert entry(None, C.byref(qp), fake, 48, 1, None, None, None) == SC_EINVAL
        res = pkg.make_polish_poses_params(); res.reserved[1] = 1
        for bad in (pkg.ScPolishPosesParams(31, 16, 0, 0, 0), pkg.make_polish_poses_params(max_iter=0), pkg.make_polish_poses_params(max_iter=65),
                    pkg.make_polish_poses_params(sel_mode=4), pkg.make_polish_poses_params(sel_mode=1), pkg.make_polish_poses_params(sel_mode=3),
                    pkg.make_polish_poses_params(label0=1), pkg.make_polish_poses_params(flags=2), res):
            assert entry(None, C.byref(bad), fake, 64, 1, None, fake, None) == SC_EINVAL


# ---- the scenes are what the GPU tests use them for: asserted on the reference alone ---------------------------------------------
def test_the_sizes_and_that_every_chunk_holds_an_inlier(pkg, O):
    assert PF.SIZES == (65, 129, 512, 7400)
    nch = (max(PF.SIZES) + 63) // 64
    assert nch == 116 and 9 * nch > 1024 >= 7 * nch  # pass 2, and pass 2 alone, needs a second round of the deal (from 114 chunks on)
    for n in PF.SIZES[:3]:
        sc = PF.scene(pkg, n)
        Rt = PF.rt_of(sc.R_gt, sc.t_gt)
        mask = O.mask(sc.src, sc.tgt, Rt, PF.TAU)
        assert all(mask[lo: lo + 64].any() for lo in range(0, n, 64)), n  # (the last, partial chunk included)
        rec, m = PF.one(O, sc.src, sc.tgt, Rt, PF.TAU)
        print(n, int(rec["score0"]), int(rec["score"]), int(rec["iters"]), int(rec["stop"]))
        assert int(rec["status"]) == SC_OK and int(rec["score"]) == int(m.sum()) >= 3 and int(rec["iters"]) >= 1
        # no selection: the reference IS polish_ref.iterate
        rt, iters, stop = polish_ref.iterate(O, sc.src, sc.tgt, Rt, PF.TAU, 16)
        assert rt.tobytes() == rec["Rt"].tobytes() and iters == int(rec["iters"])
        assert {"fixed": PF.STOP_FIXED, "declined": PF.STOP_DECLINED, "max_iter": PF.STOP_MAX_ITER}[stop] == int(rec["stop"])


def test_the_crafted_labels_give_pose_1_three_nested_sets(pkg, O):
    sc, label = PF.motions(pkg)
    assert len(sc.src) == 1500 and len(sc.motions) == 2
    own = np.flatnonzero(sc.label == 1)
    assert len(own) == 225 and (label[own[0::3]] == -1).all() and (label[own[1::3]] == 0).all() and (label[own[2::3]] == 1).all()
    assert np.array_equal(np.delete(label, own), np.delete(sc.label, own))
    poses = [PF.rt_of(R, t) for R, t in sc.motions]
    got = {}
    for name, mode in (("none", PF.SEL_NONE), ("alive", PF.SEL_ALIVE), ("label", PF.SEL_LABEL)):
        recs, masks = PF.poses(O, sc.src, sc.tgt, poses, PF.TAU, mode, None if mode == PF.SEL_NONE else label)
        print(name, recs["score0"].tolist(), recs["score"].tolist(), recs["iters"].tolist(), recs["stop"].tolist())
        assert (recs["status"] == SC_OK).all() and (masks.sum(axis=1) >= 3).all() and (recs["score"] >= 3).all()  # every selection keeps >= 3 inliers
        got[name] = (recs[1], masks[1])
    for a, b in (("none", "alive"), ("none", "label"), ("alive", "label")):  # pairwise different records for pose 1 ...
        assert got[a][0].tobytes() != got[b][0].tobytes(), (a, b)
        assert got[a][0]["Rt"].tobytes() != got[b][0]["Rt"].tobytes(), (a, b)
    # ... over nested inlier sets (a correspondence of motion 1 is far from every other pose's reach, so the sets are those of the labels)
    assert int(got["label"][1].sum()) < int(got["alive"][1].sum()) < int(got["none"][1].sum())
    assert (label[np.flatnonzero(got["alive"][1])] == -1).any()  # ALIVE admits what LABEL cannot: an index labelled -1
    assert not (label[np.flatnonzero(got["alive"][1])] == 0).any()
    # label0 shifted with the labels gives the same records; SEL_MASK with the ALIVE set of pose 1 gives pose 1's ALIVE record
    for mode in (PF.SEL_LABEL, PF.SEL_ALIVE):
        a = PF.poses(O, sc.src, sc.tgt, poses, PF.TAU, mode, label)
        b = PF.poses(O, sc.src, sc.tgt, poses, PF.TAU, mode, label + 7, label0=7)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    alive1 = PF.part_of(1500, 1, PF.SEL_ALIVE, label).astype(np.uint8)
    assert PF.poses(O, sc.src, sc.tgt, poses[1:], PF.TAU, PF.SEL_MASK, alive1)[0][0].tobytes() == got["alive"][0].tobytes()
    # the wrapping add: label0 = INT32_MAX, k = 1 -> want = INT32_MIN: ALIVE admits every label, LABEL only INT32_MIN
    assert PF.part_of(4, 1, PF.SEL_ALIVE, np.array([-5, 0, 2**31 - 1, -2**31], np.int32), 2**31 - 1).all()
    assert PF.part_of(4, 1, PF.SEL_LABEL, np.array([-5, 0, 2**31 - 1, -2**31], np.int32), 2**31 - 1).tolist() == [False, False, False, True]


def test_a_far_pose_is_declined_and_the_status_rules(pkg, O):
    sc = PF.scene(pkg, 129)
    Rt = PF.rt_of(sc.R_gt, sc.t_gt)
    far = PF.far(Rt)
    rec, mask = PF.one(O, sc.src, sc.tgt, far, PF.TAU)
    assert int(rec["status"]) == SC_OK and rec["Rt"].tobytes() == far.tobytes() and int(rec["stop"]) == PF.STOP_DECLINED
    assert (int(rec["iters"]), int(rec["score0"]), int(rec["score"]), int(mask.sum())) == (0, 0, 0, 0)
    good = PF.one(O, sc.src, sc.tgt, Rt, PF.TAU)
    bad = Rt.copy(); bad[4] = np.inf
    recs, masks = PF.poses(O, sc.src, sc.tgt, [Rt, Rt, bad, Rt], PF.TAU, statuses=[SC_OK, PF.SC_ENOHYP, SC_OK, 77])
    none = np.zeros((), PF.RESULT_DTYPE); none["Rt"], none["stop"] = PF.IDENT, PF.STOP_DECLINED
    assert recs[0].tobytes() == good[0].tobytes() and np.array_equal(masks[0], good[1])
    for k, st in ((1, PF.SC_ENOHYP), (2, SC_EINVAL), (3, 77)):
        none["status"] = st
        assert recs[k].tobytes() == none.tobytes() and not masks[k].any()
    # without the flag the word at byte 48 is not a status
    assert PF.poses(O, sc.src, sc.tgt, [Rt], PF.TAU)[0][0].tobytes() == good[0].tobytes()
    # the truncated score modes score the participating rows only
    part = np.arange(129) % 2 == 0
    for mode in (1, 2):
        r, m = PF.one(O, sc.src, sc.tgt, Rt, PF.TAU, part, score_mode=mode)
        full = PF.one(O, sc.src, sc.tgt, Rt, PF.TAU, score_mode=mode)[0]
        assert 0 < int(r["score0"]) < int(full["score0"]) and not m[~part].any()
