"""GPU: correspondences of a batch's problems labelled by the pose that fits best (include/saccot.h, sc_assign_poses_batch /
sc_assign_poses_batch_device).

The expected value of every case is tests/assign_ref.py per problem, and every comparison is bit for bit: every label and the 32
bytes of every record.  GPU against GPU as well: the frame form on the same problem, and FIRST on the records of
sc_register_instances_batch_device against that call's labels and counts.
"""
import ctypes as C

import numpy as np
import pytest

import assign_ref as AR
import instances_batch_ref as IB

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
SIZES = ((3, 1.0), (64, .4), (65, .4), (512, .3))  # (n, rho): the smallest problem, one bit word and a bit, the maximum
REC = 32


def _params(pkg, soa=False, **kw):
    return pkg.make_params(**AR.kw_of(), layout=pkg.SC_SOA if soa else pkg.SC_AOS, **kw)


def _scenes(pkg):
    return [pkg.synth.make_scene(n, rho, 1.0, AR.TAU, 7600 + n) for n, rho in SIZES]


def _pack(scenes, soa=False):
    src, tgt = np.concatenate([s.src for s in scenes]), np.concatenate([s.tgt for s in scenes])
    offset = np.concatenate([[0], np.cumsum([len(s.src) for s in scenes])]).astype(np.uint32)
    if soa:
        src, tgt = np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)
    return src, tgt, offset


def _poses(pkg, scenes, K, dtype=None):
    """(K, B) pose records, motion-major: neighbours of every problem's own motion, far poses and a copy among them (assign_ref.many),
    and — from K = 16 on — a plane of SC_ENOHYP and a non-finite pose"""
    pose = np.zeros((K, len(scenes)), dtype or pkg.BATCH_RESULT_DTYPE)
    for b, s in enumerate(scenes):
        gt = AR.rt_of(s.R_gt, s.t_gt)
        pose["Rt"][:, b] = AR.many(gt, K, 500 + b) if K > 2 else np.concatenate([gt[None, :], AR.perturbed(gt, 1, 9 + b)])[:K]
    if K >= 16:
        pose["status"][2, :] = SC_ENOHYP
        pose["Rt"][4, 1][5] = np.nan
    return pose


def _assert_batch(got, exp, offset, what=""):
    (gl, gr), (el, er) = got, exp
    for b in range(len(offset) - 1):
        lo, hi = int(offset[b]), int(offset[b + 1])
        print(what, "problem", b, gr["count"][:6, b].tolist(), "expected", er["count"][:6, b].tolist())
        assert np.array_equal(gl[lo:hi], el[b]), (what, b)
        assert np.ascontiguousarray(gr[:, b]).tobytes() == np.ascontiguousarray(er[:, b]).tobytes(), (what, b)


@pytest.mark.parametrize("K,soa", [(1, False), (2, False), (16, False), (16, True), (64, False)])
def test_the_batch_equals_the_reference_and_the_frame_form(pkg, O, reg, K, soa):
    scenes = _scenes(pkg)
    problems = [(s.src, s.tgt) for s in scenes]
    src, tgt, offset = _pack(scenes, soa)
    p = _params(pkg, soa)
    pose = _poses(pkg, scenes, K)
    got = {}
    for mode in (AR.BEST, AR.FIRST):
        got[mode] = reg.assign_poses_batch(src, tgt, offset, p, pose, mode=mode)
        _assert_batch(got[mode], AR.batch(O, problems, pose["Rt"], AR.TAU, mode, pose["status"]), offset, f"K={K} soa={soa} mode={mode}")
        assert not got[mode][1]["reserved"].any()
        assert np.array_equal(got[mode][1]["score"], got[mode][1]["count"])
    if K >= 16:
        assert (got[AR.BEST][1]["status"][2] == SC_ENOHYP).all() and int(got[AR.BEST][1]["status"][4, 1]) == SC_EINVAL
        assert not got[AR.BEST][1]["count"][2].any() and int(got[AR.BEST][1]["count"][4, 1]) == 0
    if K == 16 and not soa:  # the device form, stride 64 (sc_polish_batch_result): the same bytes
        import torch
        pose64 = _poses(pkg, scenes, K, pkg.api.POLISH_BATCH_RESULT_DTYPE)
        d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
        d_pose = torch.from_numpy(pose64.view(np.uint8).reshape(-1).copy()).cuda()
        d_label = torch.full((int(offset[-1]),), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
        d_asg = torch.full((K * len(scenes) * REC,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        reg.assign_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, pkg.make_assign_params(), d_pose.data_ptr(), 64, K,
                                      d_label.data_ptr(), d_asg.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_label.cpu().numpy(), got[AR.BEST][0]) and d_asg.cpu().numpy().tobytes() == got[AR.BEST][1].tobytes()
        assert d_pose.cpu().numpy().tobytes() == pose64.tobytes()  # d_pose is read, never written
    # the frame form on the same problem (it ends nothing; the batch call above ended every frame, so each problem is registered first)
    if K in (2, 64):
        framed = 0
        for b, s in enumerate(scenes):
            if reg.register(s.src, s.tgt, params=_params(pkg))["status"] != SC_OK:
                continue  # (SC_ENOHYP leaves no frame: a problem of three correspondences may hold no triangle)
            framed += 1
            lo, hi = int(offset[b]), int(offset[b + 1])
            for mode in (AR.BEST, AR.FIRST):
                lab, _, rec = reg.assign_poses_frame(np.ascontiguousarray(pose[:, b]), mode=mode, flags=pkg.SC_ASSIGN_STATUS)
                assert np.array_equal(lab, got[mode][0][lo:hi]), (b, mode)
                assert rec.tobytes() == np.ascontiguousarray(got[mode][1][:, b]).tobytes(), (b, mode)
        assert framed >= 3


def test_first_on_the_instances_batch_records_reproduces_its_labels(pkg, O, reg):
    import torch
    problems = IB.scenes(pkg)
    B, K = len(problems), 4
    src, tgt = np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems])
    offset = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.uint32)
    total = int(offset[-1])
    p = pkg.make_params(**IB.KW, max_triangles=AR.kw_of()["max_triangles"])
    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    d_res = torch.zeros(K * B * 80, dtype=torch.uint8, device="cuda")
    d_label = torch.zeros(total, dtype=torch.int32, device="cuda"); d_nfound = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_lab2 = torch.full((total,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
    d_asg = torch.full((K * B * REC,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    # min_score 3: a plane 0 that is SC_OK is then a found motion (its triangle's three vertices), so every plane past nfound is SC_ENOHYP
    reg.register_instances_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, K, 3, d_res.data_ptr(), d_label.data_ptr(),
                                        d_nfound.data_ptr())
    reg.assign_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, pkg.make_assign_params(mode=AR.FIRST), d_res.data_ptr(), 80, K,
                                  d_lab2.data_ptr(), d_asg.data_ptr())
    torch.cuda.synchronize()
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE).reshape(K, B)
    asg = np.frombuffer(d_asg.cpu().numpy().tobytes(), pkg.ASSIGN_RESULT_DTYPE).reshape(K, B)
    nfound = d_nfound.cpu().numpy()
    print("nfound", nfound.tolist(), "counts", asg["count"].T.tolist())
    assert np.array_equal(d_lab2.cpu().numpy(), d_label.cpu().numpy()) and nfound.max() >= 2
    for b in range(B):
        for k in range(K):
            if k < nfound[b]:
                assert int(asg[k, b]["status"]) == SC_OK and int(asg[k, b]["count"]) == int(res[k, b]["best_count"]) == int(asg[k, b]["score"])
            else:  # a plane without a motion is passed through and claims nothing
                assert int(asg[k, b]["status"]) == int(res[k, b]["status"]) != SC_OK and int(asg[k, b]["count"]) == 0
    labels, exp = AR.batch(O, problems, res["Rt"], IB.KW["tau"], AR.FIRST, res["status"])
    assert asg.tobytes() == exp.tobytes()


def test_a_nan_coordinate_is_einval_alone_and_position_does_not_matter(pkg, O, reg):
    scenes = _scenes(pkg)
    K = 16
    pose = _poses(pkg, scenes, K)
    p = _params(pkg)
    src, tgt, offset = _pack(scenes)
    clean = reg.assign_poses_batch(src, tgt, offset, p, pose)
    bad_tgt = tgt.copy(); bad_tgt[int(offset[2]) + 7, 1] = np.nan  # problem 2
    lab, rec = reg.assign_poses_batch(src, bad_tgt, offset, p, pose)
    lo, hi = int(offset[2]), int(offset[3])
    assert (lab[lo:hi] == -1).all() and (rec["status"][:, 2] == SC_EINVAL).all() and not rec["count"][:, 2].any() and not rec["score"][:, 2].any()
    keep = np.ones(len(lab), bool); keep[lo:hi] = False
    assert np.array_equal(lab[keep], clean[0][keep])
    for b in (0, 1, 3):
        assert np.ascontiguousarray(rec[:, b]).tobytes() == np.ascontiguousarray(clean[1][:, b]).tobytes()
    problems = [(s.src, s.tgt) for s in scenes]
    problems[2] = (scenes[2].src, bad_tgt[lo:hi])
    _assert_batch((lab, rec), AR.batch(O, problems, pose["Rt"], AR.TAU, AR.BEST, pose["status"]), offset, "a NaN in problem 2")
    # position independence: problem 3 first, last and alone, in batches of 6, 2 and 1 problems: the same bytes
    order = [3, 0, 1, 2, 1, 3]
    s6, t6, o6 = _pack([scenes[b] for b in order])
    l6, r6 = reg.assign_poses_batch(s6, t6, o6, p, np.ascontiguousarray(pose[:, order]))
    for pos, b in enumerate(order):
        assert np.array_equal(l6[int(o6[pos]): int(o6[pos + 1])], clean[0][int(offset[b]): int(offset[b + 1])]), pos
        assert np.ascontiguousarray(r6[:, pos]).tobytes() == np.ascontiguousarray(clean[1][:, b]).tobytes(), pos
    s1, t1, o1 = _pack([scenes[3]])
    l1, r1 = reg.assign_poses_batch(s1, t1, o1, p, np.ascontiguousarray(pose[:, 3:4]))
    assert np.array_equal(l1, clean[0][int(offset[3]):]) and r1.tobytes() == np.ascontiguousarray(clean[1][:, 3:4]).tobytes()


def test_refusals_name_their_reason_and_the_entry_ends_the_frame(pkg, O):
    L = pkg.load_library()
    scenes = _scenes(pkg)
    src, tgt, offset = _pack(scenes)
    B = len(scenes)
    r = pkg.Registrar(0)
    try:
        pose = _poses(pkg, scenes, 2)
        label = np.zeros(int(offset[-1]), np.int32); asg = np.zeros((2, B), AR.RESULT_DTYPE)
        p = _params(pkg)
        f32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        u32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731

        def call(ap, stride=80, k=2, offset=offset, p=p, pose=pose, label=label, asg=asg, src=src):
            nb = 0 if offset is None else len(offset) - 1
            rc = L.sc_assign_poses_batch(r._h, f32(src), f32(tgt), u32(offset), nb, None if p is None else C.byref(p),
                                         None if ap is None else C.byref(ap), vp(pose), stride, k, vp(label), vp(asg))
            return rc, L.sc_last_error(r._h).decode()

        ok = pkg.make_assign_params()
        assert call(ok)[0] == SC_OK
        good = (label.copy(), asg.copy())
        _assert_batch(good, AR.batch(O, [(s.src, s.tgt) for s in scenes], pose["Rt"], AR.TAU, AR.BEST, pose["status"]), offset, "good")
        short = pkg.make_assign_params(); short.size = 36
        res = pkg.make_assign_params(); res.reserved[0] = 1
        mk = pkg.make_assign_params
        big = offset.copy(); big[-1] += 1  # the last problem: 513 correspondences
        cases = {
            "ap NULL": (lambda: call(None), "NULL"),
            "src NULL": (lambda: call(ok, src=None), "NULL"),
            "params NULL": (lambda: call(ok, p=None), "NULL"),
            "pose NULL": (lambda: call(ok, pose=None), "NULL"),
            "label NULL": (lambda: call(ok, label=None), "NULL"),
            "asg NULL": (lambda: call(ok, asg=None), "NULL"),
            "size": (lambda: call(short), "size"),
            "mode 2": (lambda: call(mk(mode=2)), "mode"),
            "a mask": (lambda: call(mk(sel_mode=1)), "sel_mode"),
            "flag 2": (lambda: call(mk(flags=2)), "flag"),
            "reserved": (lambda: call(res), "reserved"),
            "n_poses 0": (lambda: call(ok, k=0), "n_poses"),
            "n_poses 65": (lambda: call(ok, k=65), "n_poses"),
            "stride 48": (lambda: call(ok, stride=48), "pose_stride"),
            "stride 54": (lambda: call(ok, stride=54), "pose_stride"),
            "a problem of 513": (lambda: call(ok, offset=big), "sc_assign_poses_batch"),
            "sharded params": (lambda: call(ok, p=_params(pkg, shard_world=2)), "sc_assign_poses_batch"),
        }
        for what, (fn, word) in cases.items():
            rc, text = fn()
            print(what, rc, text)
            assert rc == SC_EINVAL and word in text and "sc_assign_poses_batch" in text, what
        assert call(ok)[0] == SC_OK and np.array_equal(label, good[0]) and asg.tobytes() == good[1].tobytes()
        assert call(mk(flags=1))[0] == SC_OK and asg.tobytes() == good[1].tobytes()  # the flag changes nothing: the status is always read
        # like every batch entry it ends the frame a context holds
        f = r.register(scenes[3].src, scenes[3].tgt, params=p)
        assert f["status"] == SC_OK and r.peel()["status"] in (SC_OK, SC_ENOHYP)
        assert call(ok)[0] == SC_OK
        with pytest.raises(pkg.SacCotError) as e:
            r.peel()
        assert e.value.status == SC_EINVAL and "no frame" in str(e.value)
    finally:
        r.close()
