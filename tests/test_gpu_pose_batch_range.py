"""GPU: sc_pose_info_batch (plain, slot and pairs forms) and sc_assign_poses on a batch at the ends of the fp32 range.

tests/test_gpu_pose_info.py sees one crafted problem at +-3e38 and tests/test_gpu_assign_batch.py nothing of the range.  Here the
problems are those of tests/test_gpu_batch_range.py (n = 192, 300, 512: coordinates and parameters times 2^k for k from -70 to 70,
far from the origin, rows at +-3e38, shrunk blocks, parameters at the ends of what is accepted), packed by launch, and the
all-magnitudes-in-one-launch batch in which a workgroup at 2^-70 runs beside one at 2^70.  The input poses are the reference's batch
records and the table of shifted and hostile poses of tests/test_batch_tail_range_ref.py — ZEROS (sums that are exactly 0 under a count
that is not) and E_MIRROR (entries near 1e77) among them; the assign lists hold 1, 3, 16 and 64 poses per problem, motion-major, with
hostile poses and switched-off records between good ones.

tests/test_pose_range_ref.py owns the cases and the expected values (tests/pose_info_ref.py, tests/assign_ref.py) and asserts on the
references alone that they are what they are used for.  Every comparison is bit for bit: the 320 bytes of every information record,
every label, the 32 bytes of every assign record.  No tolerances.
"""
import numpy as np
import pytest

import assign_ref as AR
import batch_ref
import pose_info_ref as PI
import test_batch_range_ref as R
import test_batch_tail_range_ref as TR
import test_pose_range_ref as P
from test_gpu_assign_batch import _assert_batch
from test_gpu_pose_info import _assert_info, _junk_info, _records
from test_range_oracle import UNIT

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5


def _pack(problems, soa=False):
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.uint32)
    src, tgt = np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems])
    if soa:
        src, tgt = np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)
    return src, tgt, off


def _params(pkg, kw, soa=False, **more):
    return pkg.make_params(**kw, layout=pkg.SC_SOA if soa else pkg.SC_AOS, **more)


def _info_device(pkg, reg, src, tgt, off, p, pose):
    import torch
    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    d_pose = torch.from_numpy(np.frombuffer(pose.tobytes(), np.uint8).copy()).cuda()
    d_info = _junk_info(torch, len(off) - 1)
    torch.cuda.synchronize()
    reg.pose_info_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_pose.data_ptr(), pose.dtype.itemsize, d_info.data_ptr())
    torch.cuda.synchronize()
    assert d_pose.cpu().numpy().tobytes() == pose.tobytes()              # d_pose is read, never written
    return _records(pkg, d_info)


# ---- 1: sc_pose_info_batch, packed by launch, both layouts, host form and device form ------------------------------------------------
@pytest.mark.parametrize("gid", list(P.INFO_LAUNCHES))
def test_pose_info_equals_the_reference_at_the_ends_of_the_range(pkg, O, reg, gid):
    kw, cases = P.INFO_LAUNCHES[gid]
    refs = [P.info_case(pkg, O, name, pose) for name, pose in cases]
    problems = [(r[0], r[1]) for r in refs]
    rin = np.array([r[3] for r in refs], batch_ref.RESULT_DTYPE)
    exp = np.array([r[4] for r in refs], PI.RESULT_DTYPE)
    assert len(problems) <= 40 and max(len(s) for s, _ in problems) <= 512
    seen = None
    for soa in (False, True):
        src, tgt, off = _pack(problems, soa)
        p = _params(pkg, kw, soa)
        got = reg.pose_info_batch_raw(src, tgt, off, p, rin)
        _assert_info(got, exp, f"{gid} soa={soa}")
        assert _info_device(pkg, reg, src, tgt, off, p, rin).tobytes() == got.tobytes(), (gid, soa)
        seen = seen or got.tobytes()
        assert got.tobytes() == seen                                     # the layout of the points does not matter
    # ... and alone: a record is a function of its own problem, its pose and tau
    for b in range(0, len(cases), max(1, len(cases) // 6)):
        s, t, o = _pack(problems[b: b + 1])
        assert reg.pose_info_batch_raw(s, t, o, _params(pkg, kw), rin[b: b + 1]).tobytes() == exp[b: b + 1].tobytes(), (gid, cases[b])


def test_pose_info_of_all_magnitudes_in_one_launch(pkg, O, reg):
    """Workgroups side by side at 2^-70 .. 2^70, 2^24 from the origin and at +-3e38, under the unit parameters."""
    problems, rin, exp = P.info_one_launch(pkg, O)
    kw = dict(UNIT, max_triangles=R.T)
    for soa in (False, True):
        src, tgt, off = _pack(problems, soa)
        p = _params(pkg, kw, soa)
        got = reg.pose_info_batch_raw(src, tgt, off, p, rin)
        _assert_info(got, exp, f"one launch soa={soa}")
        assert _info_device(pkg, reg, src, tgt, off, p, rin).tobytes() == got.tobytes()
    assert (got["inliers"] > 0).sum() >= 8


# ---- 2: the slot form and the pairs form -------------------------------------------------------------------------------------------------
def test_the_slot_and_pairs_forms_on_all_magnitudes(pkg, O, reg):
    """pose_info_batch_kernel's slot and pairs jobs gather the problem through corr and take n from a device word.  The descriptors
    of problem b are rows of the identity, the target's permuted and its points permuted alike: the matcher (mutual, knn 1) returns the
    permutation, the gathered problem is problem b in its own order, and the record is the plain form's — against
    pose_info_ref.slots_one on the GPU's own corr / count, and against the plain form's bytes."""
    import torch
    problems, rin, exp = P.info_one_launch(pkg, O)
    kw = dict(UNIT, max_triangles=R.T)
    nb, D = len(problems), 512
    rng = np.random.default_rng(61)
    perm = [rng.permutation(len(s)) for s, _ in problems]                 # target row j holds the partner of source row perm[j]
    eye = np.eye(D, dtype=np.float32)
    sets = []
    for (s, t), pm in zip(problems, perm):
        sets += [(s, eye[:len(s)]), (np.ascontiguousarray(t[pm]), np.ascontiguousarray(eye[pm]))]
    set_off = np.concatenate([[0], np.cumsum([len(a) for a, _ in sets])]).astype(np.uint32)
    mp = pkg.api.make_match_params(D, knn=1, mutual=True)
    plain = reg.pose_info_batch_raw(*_pack(problems), _params(pkg, kw), rin)
    _assert_info(plain, exp, "plain")
    d_pose = torch.from_numpy(np.frombuffer(rin.tobytes(), np.uint8).copy()).cuda()

    def check(got, corr, count, order, what):
        for pos, b in enumerate(order):
            n = len(problems[b][0])
            lo = sum(len(problems[x][0]) for x in order[:pos])
            assert count[pos].tolist() == [n, 0], (what, b)
            inv = np.argsort(perm[b])
            assert np.array_equal(corr[lo: lo + n], np.stack([np.arange(n), inv], 1)), (what, b)
            ref = PI.slots_one(O, sets[2 * b][0], sets[2 * b + 1][0], corr[lo: lo + n], n, 0, rin[b]["status"], rin[b]["Rt"], kw["tau"])
            assert got[pos].tobytes() == ref.tobytes() == plain[b].tobytes(), (what, b)

    for soa in (False, True):
        p = _params(pkg, kw, soa)
        # the slot form behind sc_match_batch_device
        so = reg._offsets([len(s) for s, _ in problems])
        lay = (lambda a: np.ascontiguousarray(a.T)) if soa else (lambda a: a)
        d_ps = torch.from_numpy(lay(np.concatenate([sets[2 * b][0] for b in range(nb)]))).cuda()
        d_pt = torch.from_numpy(lay(np.concatenate([sets[2 * b + 1][0] for b in range(nb)]))).cuda()
        d_fs = torch.from_numpy(np.concatenate([sets[2 * b][1] for b in range(nb)])).cuda()
        d_ft = torch.from_numpy(np.concatenate([sets[2 * b + 1][1] for b in range(nb)])).cuda()
        slots = int(so[-1])
        d_corr = torch.full((slots, 2), -7, dtype=torch.int32, device="cuda"); d_d2 = torch.zeros(slots, dtype=torch.float32, device="cuda")
        d_count = torch.full((nb, 2), 9, dtype=torch.int32, device="cuda")
        d_info = _junk_info(torch, nb)
        torch.cuda.synchronize()
        reg.match_batch_device(d_fs.data_ptr(), so, d_ft.data_ptr(), so, mp, d_corr.data_ptr(), d_d2.data_ptr(), d_count.data_ptr())
        reg.pose_info_batch_slots_device(d_ps.data_ptr(), so, d_pt.data_ptr(), so, 1, p, d_corr.data_ptr(), d_count.data_ptr(), d_pose.data_ptr(), 80,
                                         d_info.data_ptr())
        torch.cuda.synchronize()
        check(_records(pkg, d_info), d_corr.cpu().numpy(), d_count.cpu().numpy(), list(range(nb)), f"slots soa={soa}")
        # the pairs form behind sc_match_pairs_device: the list in reverse order, every pair under its own problem's record
        order = list(range(nb))[::-1]
        pairs = np.array([(2 * b, 2 * b + 1) for b in order], np.uint32)
        d_pts = torch.from_numpy(lay(np.concatenate([a for a, _ in sets]))).cuda()
        d_feat = torch.from_numpy(np.concatenate([f for _, f in sets])).cuda()
        d_pose_r = torch.from_numpy(np.frombuffer(rin[order].tobytes(), np.uint8).copy()).cuda()
        d_corr.fill_(-7); d_count.fill_(9)
        d_info = _junk_info(torch, nb)
        torch.cuda.synchronize()
        reg.match_pairs_device(d_feat.data_ptr(), set_off, pairs, mp, d_corr.data_ptr(), d_d2.data_ptr(), d_count.data_ptr())
        reg.pose_info_pairs_slots_device(d_pts.data_ptr(), set_off, pairs, 1, p, d_corr.data_ptr(), d_count.data_ptr(), d_pose_r.data_ptr(), 80,
                                         d_info.data_ptr())
        torch.cuda.synchronize()
        check(_records(pkg, d_info), d_corr.cpu().numpy(), d_count.cpu().numpy(), order, f"pairs soa={soa}")


# ---- 3: sc_assign_poses on a batch ------------------------------------------------------------------------------------------------------
def _assign_launch(pkg, O, reg, kw, names, score_mode, what):
    refs = {(K, mode): [P.assign_batch_one(pkg, O, name, K, mode, score_mode) for name in names] for K in P.ASSIGN_KS for mode in (AR.BEST, AR.FIRST)}
    problems = [(r[0], r[1]) for r in refs[1, AR.BEST]]
    assert len(problems) <= 40 and max(len(s) for s, _ in problems) <= 512
    for K in P.ASSIGN_KS:
        pose = np.frombuffer(bytes([0xA5]) * (80 * K * len(names)), batch_ref.RESULT_DTYPE).copy().reshape(K, len(names))   # motion-major
        for b, r in enumerate(refs[K, AR.BEST]):
            pose["Rt"][:, b], pose["status"][:, b] = r[3], r[4]
        for soa in (False, True):
            src, tgt, off = _pack(problems, soa)
            p = _params(pkg, kw, soa, score_mode=score_mode)
            for mode in (AR.BEST, AR.FIRST):
                got = reg.assign_poses_batch(src, tgt, off, p, pose, mode=mode)
                exp_rec = np.zeros((K, len(names)), AR.RESULT_DTYPE)
                for b, r in enumerate(refs[K, mode]):
                    exp_rec[:, b] = r[5][2]
                _assert_batch(got, ([r[5][0] for r in refs[K, mode]], exp_rec), off, f"{what} K={K} soa={soa} mode={mode}")
                if K == 16 and not soa:                                  # the device form: the same bytes
                    import torch
                    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
                    d_pose = torch.from_numpy(pose.view(np.uint8).reshape(-1).copy()).cuda()
                    d_label = torch.full((int(off[-1]),), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
                    d_asg = torch.full((K * len(names) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    reg.assign_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, pkg.make_assign_params(mode=mode), d_pose.data_ptr(), 80, K,
                                                  d_label.data_ptr(), d_asg.data_ptr())
                    torch.cuda.synchronize()
                    assert np.array_equal(d_label.cpu().numpy(), got[0]) and d_asg.cpu().numpy().tobytes() == got[1].tobytes(), (what, mode)
    return refs


@pytest.mark.parametrize("gid", list(P.ASSIGN_LAUNCHES))
def test_assign_equals_the_reference_at_the_ends_of_the_range(pkg, O, reg, gid):
    kw, names = P.ASSIGN_LAUNCHES[gid]
    _assign_launch(pkg, O, reg, kw, names, 0, gid)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", TR.MODE_NAMES)
def test_assign_in_the_truncated_score_modes(pkg, O, reg, name, mode):
    """1 / tau^2 and 1 / tau are inf (f:tau-30), 0 (f:tau25), 2^120 / 2^-120-ish (a:300:-56 / 62)"""
    _assign_launch(pkg, O, reg, TR.tail_kw(name), [name], mode, f"{name} score mode {mode}")


def test_assign_of_all_magnitudes_in_one_launch(pkg, O, reg):
    """K = 16 around each problem's own winner under the unit parameters: a workgroup at 2^-70 beside one at 2^70."""
    problems, rin, _ = P.info_one_launch(pkg, O)
    kw = dict(UNIT, max_triangles=R.T)
    K = 16
    names = R.ONE_LAUNCH
    pose = np.zeros((K, len(problems)), batch_ref.RESULT_DTYPE)
    for b, name in enumerate(names):
        rt, st = P.pose_lists(rin[b]["Rt"], P.batch_k(name), kw["tau"], P.ASSIGN_SEED, (K,), P.BATCH_HOSTILE, P.BATCH_STATUS)[K]
        pose["Rt"][:, b], pose["status"][:, b] = rt, st
    src, tgt, off = _pack(problems)
    for mode in (AR.BEST, AR.FIRST):
        with np.errstate(all="ignore"):
            exp = AR.batch(O, problems, pose["Rt"], kw["tau"], mode, pose["status"])
        got = reg.assign_poses_batch(src, tgt, off, _params(pkg, kw), pose, mode=mode)
        _assert_batch(got, exp, off, f"one launch mode={mode}")
    assert int((got[0] >= 0).sum()) > 300
