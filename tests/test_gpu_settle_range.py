"""GPU: sc_settle_poses (frame and batch forms) at the ends of the fp32 range and past one trip of its deals.

tests/test_gpu_settle_frame.py and test_gpu_settle_batch.py run the entry on unit-scale scenes of at most 1500 correspondences.
Here the frames are those of tests/test_gpu_pose_frame_range.py — test_range_oracle.scene_small times 2^k, far from the origin, with
rows at +-3e38, tau at the ends of its range, the truncated score modes (settle_scores), scene_big at k = 62 and -56 —, the batch
problems those of tests/test_gpu_pose_batch_range.py, and the shape cases hold 2048, 2049 and 2113 correspondences: a trip of
settle_label covers 32 chunks, so the last two take a second trip, whose labels settle_scores re-reads without a barrier.

tests/test_settle_merge_range_ref.py owns the cases and the expected values (tests/settle_ref.py) and asserts on the reference alone
that the cases are what they are used for.  Every comparison is bit for bit: the 64 bytes of every record, every label, the bits of
every d2, both rounds words.  No tolerances.  Every call runs in its host form and in its device form; the two must agree byte for
byte.
"""
import numpy as np
import pytest

import batch_ref
import test_batch_range_ref as R
import test_pose_range_ref as P
import test_settle_merge_range_ref as S
from conftest import nan_equal_bits
from test_gpu_pose_frame_range import _frame
from test_gpu_settle_batch import _assert_batch
from test_gpu_settle_frame import _assert_same, _device
from test_range_oracle import pow2

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
_GPU = {}  # (name, part) -> {(list, max_iter, masked): the GPU's own result}: what the metamorphic check compares


def _pose_args(pkg, rt, st):
    """a list as the call takes it: bare floats at stride 48, or records of 64 bytes under the status flag"""
    return (rt, 48, 0) if st is None else (P.records64(rt, st), 64, pkg.SC_SETTLE_STATUS)


def _settle(pkg, reg, rt, st, n, exp, max_iter, masked, what):
    """one sc_settle_poses_frame call, host form then device form, against the reference -> the host form's result"""
    pose, stride, flags = _pose_args(pkg, rt, st)
    sel_mode, sel = (pkg.SC_ASSIGN_SEL_MASK, P.third_off(n)) if masked else (pkg.SC_ASSIGN_SEL_NONE, None)
    got = reg.settle_poses_frame(pose, max_iter=max_iter, sel_mode=sel_mode, sel=sel, flags=flags)
    _assert_same(got, exp, what)
    sp = pkg.make_settle_params(max_iter=max_iter, sel_mode=sel_mode, flags=flags)
    _assert_same(_device(pkg, reg, sp, pose.tobytes(), stride, len(pose), n, sel), got, what + " device form")
    return got


def _run(pkg, O, reg, name, part):
    """one list of one frame -> what the metamorphic check keeps of it (None: the case leaves no frame)"""
    if not _frame(pkg, O, reg, name):
        assert name in S.NO_FRAME
        rt, st = P.frame_poses(pkg, O, name)
        with pytest.raises(pkg.SacCotError) as e:
            reg.settle_poses_frame(rt[:1])
        assert e.value.status == SC_EINVAL and "no frame" in str(e.value), name
        return None
    assert name not in S.NO_FRAME
    n = len(P.frame_case(pkg, O, name)[0])
    rt, st = S.frame_lists(pkg, O, name)[part]
    keep = {}
    for which, max_iter, masked in S.settle_runs(name, part):
        exp = S.settle_ref(pkg, O, name, which, max_iter, masked)
        keep[which, max_iter, masked] = _settle(pkg, reg, rt, st, n, exp, max_iter, masked, f"{name} settle {which} max_iter={max_iter} mask={masked}")
    return keep


CASES = [(name, part) for name in S.FRAME_CASES for part in S.settle_parts(name)]


@pytest.mark.parametrize("name,part", CASES)
def test_settle_equals_its_reference_at_the_ends_of_the_range(pkg, O, reg, name, part):
    keep = _run(pkg, O, reg, name, part)
    assert (keep is None) == (name in S.NO_FRAME)
    if keep is None:
        return                                                           # (only the cases test_pose_range_ref.NO_FRAME names come here)
    _GPU[name, part] = keep
    if P.frame_in_window(name) and not name.startswith("big:"):          # the case is not trivial on the GPU either
        rec, lab, d2, rounds = keep[part, 16, False]
        assert int((lab >= 0).sum()) >= 100 and rounds[0] >= 8 and rec["iters"].any()


@pytest.mark.parametrize("score_mode", [0, 2])
@pytest.mark.parametrize("n", S.SHAPE_NS)
def test_settle_past_one_trip_of_the_label_deal(pkg, O, reg, n, score_mode):
    """n = 2049, 2113: chunks 32 and 33 are a second trip of settle_label (1024 threads: 32 chunks a trip); in score mode 2 every
    tally goes through settle_scores, which re-reads the labels its own lane stored"""
    sc = S.shape_scene(pkg, n)
    kw, frame = S.shape_frame(pkg, O, n, score_mode)
    f = reg.register(sc.src, sc.tgt, params=pkg.make_params(**kw, score_mode=score_mode, flags=pkg.SC_FLAG_EXACT_TOTAL))
    assert f["status"] == frame["rc"] == SC_OK and np.array_equal(f["mask"], frame["mask"])
    assert nan_equal_bits(f["R"], frame["R"]) and nan_equal_bits(f["t"], frame["t"])
    poses = S.shape_poses(pkg, n, S.SHAPE_K_SETTLE)
    for max_iter in (16, 2):
        exp = S.shape_settle_ref(pkg, O, n, score_mode, max_iter)
        got = _settle(pkg, reg, poses, None, n, exp, max_iter, False, f"n={n} score_mode={score_mode} max_iter={max_iter}")
    assert int((got[1] >= 0).sum()) >= 600


@pytest.mark.parametrize("gid", list(S.BATCH_LAUNCHES))
def test_the_batch_form_equals_its_reference_at_the_ends_of_the_range(pkg, O, reg, gid):
    kw, names = S.BATCH_LAUNCHES[gid]
    for K, max_iter in S.SETTLE_BATCH_RUNS:
        _, problems, rt, st = S.batch_input(pkg, O, gid, K)
        exp = S.settle_batch_ref(pkg, O, gid, K, max_iter)
        assert len(problems) <= 40 and max(len(s) for s, _ in problems) <= 512
        pose = np.frombuffer(bytes([0xA5]) * (80 * K * len(names)), batch_ref.RESULT_DTYPE).copy().reshape(K, len(names))   # motion-major
        pose["Rt"], pose["status"] = rt, st
        off = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.uint32)
        src, tgt = np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems])
        for soa in (False, True):
            a, b = (np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)) if soa else (src, tgt)
            p = pkg.make_params(**kw, layout=pkg.SC_SOA if soa else pkg.SC_AOS)
            got = reg.settle_poses_batch(a, b, off, p, pose, max_iter=max_iter)
            _assert_batch(got, exp, off, f"{gid} K={K} max_iter={max_iter} soa={soa}")
        if K == S.SETTLE_BATCH_MAX_POSES:                                # the device form at stride 80: the same bytes
            import torch
            d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
            d_pose = torch.from_numpy(pose.view(np.uint8).reshape(-1).copy()).cuda()
            d_pol = torch.full((K * len(names) * 64,), 0xAB, dtype=torch.uint8, device="cuda")
            d_label = torch.full((int(off[-1]),), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
            d_rounds = torch.full((2 * len(names),), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            reg.settle_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, pkg.make_params(**kw), pkg.make_settle_params(max_iter=max_iter),
                                          d_pose.data_ptr(), 80, K, d_pol.data_ptr(), d_label.data_ptr(), d_rounds.data_ptr())
            torch.cuda.synchronize()
            assert d_pol.cpu().numpy().tobytes() == exp[0].tobytes() and np.array_equal(d_label.cpu().numpy(), np.concatenate(exp[1])), (gid, max_iter)
            assert d_rounds.cpu().numpy().view(np.uint32).tobytes() == exp[2].tobytes(), (gid, max_iter)


def test_inside_the_window_the_gpu_equals_itself_at_unit_scale(pkg, O, reg):
    """Without the reference: at the k of test_batch_range_ref.polish_metamorphic_ks labels, statuses, score0, score, iters, stop,
    rounds and R's bits are those at k = 0, t is multiplied by 2^k and d2 by 2^2k exactly (tests/test_settle_merge_range_ref.py: the
    reference is covariant on these lists at these k)."""
    def gpu(k):
        name, out = f"a:{k}", {}
        for part in S.SETTLE_PARTS:
            if (name, part) not in _GPU:
                _GPU[name, part] = _run(pkg, O, reg, name, part)
            out.update(_GPU[name, part])
        return out
    g0 = gpu(0)
    ks = R.polish_metamorphic_ks()
    assert len(ks) >= 3
    for k in ks:
        g, f = gpu(k), pow2(k)
        for run in S.SETTLE_RUNS:
            (rec, lab, d2, rounds), (rec0, lab0, d20, rounds0) = g[run], g0[run]
            rows = S.scaling_rows(run[0], len(rec))
            assert np.array_equal(lab, lab0) and rounds.tolist() == rounds0.tolist() and int((lab0 >= 0).sum()) >= 60, (k, run)
            for field in ("status", "score0", "score", "iters", "stop"):
                assert np.array_equal(rec[field], rec0[field]), (k, run, field)
            assert rec["Rt"][:, :9].tobytes() == rec0["Rt"][:, :9].tobytes(), (k, run)
            assert rec["Rt"][rows][:, 9:].tobytes() == (rec0["Rt"][rows][:, 9:] * f).tobytes() and rec0["iters"][rows].any(), (k, run)
            with np.errstate(all="ignore"):
                want = np.where(lab0 >= 0, d20 * f * f, np.float32(np.inf)).astype(np.float32)
            assert d2.tobytes() == want.tobytes(), (k, run)
