"""GPU: sc_polish_poses, sc_pose_info_frame and sc_assign_poses on a frame at the ends of the fp32 range.

tests/test_gpu_polish_poses.py, test_gpu_pose_info_frame.py and test_gpu_assign_frame.py run these entries on unit-scale scenes (the
assign kernel also at k = +-40).  Here the frames are those of tests/test_gpu_polish_range.py — test_range_oracle.scene_small times
2^k, far from the origin, with rows at +-3e38, tau at the ends of its range, the truncated score modes — plus scene_big (n = 1500: the
chain deal and the tiles of 512 see more than one round) at k = 62 and k = -56, and the poses are caller data: the winner shifted by
fractions of tau, hostile finite poses, non-finite ones, records whose status switches them off.

tests/test_pose_range_ref.py owns the cases and the expected values (tests/polish_poses_ref.py, pose_info_frame_ref.py, assign_ref.py)
and asserts on the references alone that the cases are what they are used for.  Every comparison is bit for bit: the 64 bytes of every
polish record and every mask byte, the 320 bytes of every information record, every label, the bits of every d2, the 32 bytes of every
assign record.  No tolerances.  Every call runs in its host form and in its device form; the two must agree byte for byte.
"""
import numpy as np
import pytest

import assign_ref as AR
import polish_poses_ref as PP
import pose_info_frame_ref as PIF
import test_batch_range_ref as R
import test_pose_range_ref as P
from conftest import nan_equal_bits
from test_gpu_assign_frame import _assert_same as _assert_assign
from test_gpu_assign_frame import _device as _assign_device
from test_gpu_polish_poses import _assert_pol
from test_gpu_polish_poses import _device as _polish_device
from test_gpu_pose_info_frame import _assert_info
from test_gpu_pose_info_frame import _device as _info_device
from test_range_oracle import pow2

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
_GPU = {}  # (name, part) -> what the metamorphic check compares: the GPU's own results at max_iter 16 without a selection


def _frame(pkg, O, reg, name):
    """sc_register on the case -> True if the context now holds its frame (checked against the restatement's)"""
    src, tgt, kw, mode, frame = P.frame_case(pkg, O, name)
    f = reg.register(src, tgt, params=pkg.make_params(**kw, score_mode=mode, flags=pkg.SC_FLAG_EXACT_TOTAL))
    print(name, "frame", f["status"], f["stats"]["best_rank"], f["stats"]["best_count"], "| restatement", frame["rc"], frame["best_rank"], frame["best_count"])
    assert f["status"] == frame["rc"], name
    assert np.array_equal(f["mask"], frame["mask"]) and nan_equal_bits(f["R"], frame["R"]) and nan_equal_bits(f["t"], frame["t"]), name
    return f["status"] == SC_OK


def _sel(n, sel_mode):
    return None if sel_mode == PP.SEL_NONE else P.third_off(n) if sel_mode == PP.SEL_MASK else P.crafted_label(n)


def _polish(pkg, O, reg, name, max_iter, sel_mode, with_status=True):
    """one sc_polish_poses call, host form then device form, against the reference -> the host form's (records, masks)"""
    n = len(P.frame_case(pkg, O, name)[0])
    rt, st = P.frame_poses(pkg, O, name)
    pose, stride, flags = (P.records64(rt, st), 64, pkg.SC_POLISH_POSES_STATUS) if with_status else (rt[:len(P.POLISH_POSES)], 48, 0)
    what = f"{name} polish max_iter={max_iter} sel={sel_mode} status={with_status}"
    got = reg.polish_poses(pose, max_iter=max_iter, sel_mode=sel_mode, sel=_sel(n, sel_mode), flags=flags)
    _assert_pol(got, P.polish_ref(pkg, O, name, max_iter, sel_mode, with_status), what)
    qp = pkg.make_polish_poses_params(max_iter=max_iter, sel_mode=sel_mode, flags=flags)
    dev = _polish_device(pkg, reg, qp, pose.tobytes(), stride, len(pose), n, _sel(n, sel_mode))
    assert dev[0].tobytes() == got[0].tobytes() and np.array_equal(dev[1], got[1]), what
    return got


def _info(pkg, O, reg, name, which, sel_mode):
    n = len(P.frame_case(pkg, O, name)[0])
    pose = P.info_poses(pkg, O, name, which)
    what = f"{name} info {which} sel={sel_mode}"
    got = reg.pose_info_frame(pose, sel_mode=sel_mode, sel=_sel(n, sel_mode), flags=pkg.SC_POSE_INFO_STATUS)
    _assert_info(got, P.info_ref(pkg, O, name, which, sel_mode), what)
    ip = pkg.make_pose_info_params(sel_mode=sel_mode, flags=pkg.SC_POSE_INFO_STATUS)
    assert _info_device(pkg, reg, ip, pose.tobytes(), 64, len(pose), _sel(n, sel_mode)).tobytes() == got.tobytes(), what
    return got


def _assign(pkg, O, reg, name, which, mode, sel_mode):
    n = len(P.frame_case(pkg, O, name)[0])
    rt, st = P.assign_poses(pkg, O, name)[which]
    pose, stride, flags = (rt, 48, 0) if st is None else (P.records64(rt, st), 64, pkg.SC_ASSIGN_STATUS)
    sel = None if sel_mode == AR.SEL_NONE else P.third_off(n)
    what = f"{name} assign {which} mode={mode} sel={sel_mode}"
    got = reg.assign_poses_frame(pose, mode=mode, sel_mode=sel_mode, sel=sel, flags=flags)
    _assert_assign(got, P.assign_ref(pkg, O, name, which, mode, sel_mode), what)
    ap = pkg.make_assign_params(mode=mode, sel_mode=sel_mode, flags=flags)
    dev = _assign_device(pkg, reg, ap, pose.tobytes(), stride, len(pose), n, sel)
    _assert_assign(dev, got, what + " device form")
    return got


# A frame's work is dealt over these parts, one parametrized case each (a case of scene_big's 1500 rows would otherwise take several
# times as long as any case of tests/test_gpu_polish_batch_range.py: the references are Python loops over the rows).
PARTS = ("polish", "info:in:none", "info:in:mask", "info:polished:none", "info:polished:mask", "assign:best", "assign:first")


def _run(pkg, O, reg, name, part):
    """one part of one frame -> what the metamorphic check keeps of it (None: the case leaves no frame)"""
    if not _frame(pkg, O, reg, name):
        # a frame call that returned SC_ENOHYP leaves no frame: every one of the three entries refuses
        assert name in P.NO_FRAME
        rt, st = P.frame_poses(pkg, O, name)
        for call in (lambda: reg.polish_poses(rt[:1]), lambda: reg.pose_info_frame(rt[:1]), lambda: reg.assign_poses_frame(rt[:1])):
            with pytest.raises(pkg.SacCotError) as e:
                call()
            assert e.value.status == SC_EINVAL, name
        return None
    assert name not in P.NO_FRAME
    keep = {}
    kind, *arg = part.split(":")
    if kind == "polish":
        for max_iter in P.MAX_ITERS:
            for sel_mode in (PP.SEL_NONE, PP.SEL_MASK):
                got = _polish(pkg, O, reg, name, max_iter, sel_mode)
                if max_iter == 16 and sel_mode == PP.SEL_NONE:
                    keep["polish"] = got
        _polish(pkg, O, reg, name, 16, PP.SEL_NONE, with_status=False)   # bare floats: nothing behind byte 47 is read
        if name == P.SEL_FRAME:
            for sel_mode in (PP.SEL_LABEL, PP.SEL_ALIVE):
                _polish(pkg, O, reg, name, 16, sel_mode)
    elif kind == "info":
        which, sel_mode = arg[0], PIF.SEL_NONE if arg[1] == "none" else PIF.SEL_MASK
        got = _info(pkg, O, reg, name, which, sel_mode)
        if which == "in" and sel_mode == PIF.SEL_NONE:
            keep["info"] = got
        if name == P.SEL_FRAME and sel_mode == PIF.SEL_MASK:
            _info(pkg, O, reg, name, which, PIF.SEL_LABEL)
    else:
        mode = AR.BEST if arg[0] == "best" else AR.FIRST
        for which in P.ASSIGN_LISTS:
            for sel_mode in (AR.SEL_NONE, AR.SEL_MASK):
                got = _assign(pkg, O, reg, name, which, mode, sel_mode)
                if sel_mode == AR.SEL_NONE:
                    keep["assign", which, mode] = got
    return keep


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("name", P.FRAME_CASES)
def test_the_three_entries_equal_their_references_at_the_ends_of_the_range(pkg, O, reg, name, part):
    keep = _run(pkg, O, reg, name, part)
    assert (keep is None) == (name in P.NO_FRAME)
    if keep is None:
        return                                                           # (only the cases test_pose_range_ref.NO_FRAME names come here)
    _GPU[name, part] = keep
    if P.frame_in_window(name):                                          # the case is not trivial on the GPU either
        if "polish" in keep:
            pol, masks = keep["polish"]
            assert int(pol[0]["score"]) >= 3 and masks[0].any()
        if "info" in keep:
            assert int(keep["info"][0]["inliers"]) > 0 and float(keep["info"][0]["sse"]) > 0
        if ("assign", "K65", AR.BEST) in keep:
            assert int((keep["assign", "K65", AR.BEST][0] >= 0).sum()) >= 100


def test_inside_the_window_the_gpu_equals_itself_at_unit_scale(pkg, O, reg):
    """Without the references: at the k of test_batch_range_ref.polish_metamorphic_ks labels, counts, scores, iters and R are those
    at k = 0, t is multiplied by 2^k, d2 and sse by 2^2k exactly, and the information matrix block by block by 1, 2^k and 2^2k
    (tests/test_pose_range_ref.py: the references are covariant on these poses at these k)."""
    def gpu(k):
        name, out = f"a:{k}", {}
        for part in ("polish", "info:in:none", "assign:best", "assign:first"):
            if (name, part) not in _GPU:
                _GPU[name, part] = _run(pkg, O, reg, name, part)
            out.update(_GPU[name, part])
        return out
    g0 = gpu(0)
    ks = R.polish_metamorphic_ks()
    assert len(ks) >= 3
    rows = [P.POLISH_POSES.index(p) for p in P.METAMORPHIC_POSES]
    for k in ks:
        g, f = gpu(k), pow2(k)
        (pol, masks), (pol0, masks0) = g["polish"], g0["polish"]
        for field in ("status", "score0", "score", "iters", "stop"):
            assert np.array_equal(pol[field][rows], pol0[field][rows]), (k, field)
        assert pol["Rt"][rows][:, :9].tobytes() == pol0["Rt"][rows][:, :9].tobytes(), k
        assert pol["Rt"][rows][:, 9:].tobytes() == (pol0["Rt"][rows][:, 9:] * f).tobytes(), k
        assert np.array_equal(masks[rows], masks0[rows]) and int(pol0["score"][0]) >= 3, k
        info, info0 = g["info"][rows], g0["info"][rows]
        assert np.array_equal(info["inliers"], info0["inliers"]) and np.array_equal(info["status"], info0["status"]), k
        assert info["sse"].tobytes() == (info0["sse"] * float(f) * float(f)).tobytes() and float(info0["sse"][0]) > 0, k
        m, m0 = info["info"].reshape(-1, 6, 6), info0["info"].reshape(-1, 6, 6)
        assert m[:, 3:, 3:].tobytes() == m0[:, 3:, 3:].tobytes(), k
        assert m[:, :3, 3:].tobytes() == (m0[:, :3, 3:] * float(f)).tobytes() and m[:, 3:, :3].tobytes() == (m0[:, 3:, :3] * float(f)).tobytes(), k
        assert m[:, :3, :3].tobytes() == (m0[:, :3, :3] * float(f) * float(f)).tobytes() and m0[0, :3, :3].any(), k
        for which in P.ASSIGN_LISTS:
            for mode in (AR.BEST, AR.FIRST):
                (lab, d2, rec), (lab0, d20, rec0) = g["assign", which, mode], g0["assign", which, mode]
                assert np.array_equal(lab, lab0) and rec.tobytes() == rec0.tobytes() and int((lab0 >= 0).sum()) >= 100, (k, which, mode)
                want = np.where(lab0 >= 0, d20 * f * f, np.float32(np.inf)).astype(np.float32)
                assert d2.tobytes() == want.tobytes(), (k, which, mode)
