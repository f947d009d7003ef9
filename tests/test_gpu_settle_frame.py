"""GPU: poses relabelled and refitted until stable on a scored frame (include/saccot.h, sc_settle_poses_frame /
sc_settle_poses_frame_device).

The expected value of every case is tests/settle_ref.py — rounds of tests/assign_ref.py and tests/polish_poses_ref.py composed, with
the header's stopping and record rules — and every comparison is bit for bit: the 64 bytes of every record, every label, every
residual's bits, both words of d_rounds.  No tolerances.  The equalities the header promises are checked GPU against GPU as well:
the composed loop of the existing entries, sc_polish_poses for one pose, and a settled list that goes in again.
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref
import settle_ref as SR

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
REC = 64


def _params(pkg, **kw):
    return pkg.make_params(**SR.kw_of(), **kw)


def _frame(pkg, r, src, tgt, **kw):
    """sc_register on (src, tgt): the frame the context then holds -> its result, Rt (12,) with it"""
    f = r.register(src, tgt, params=_params(pkg, **kw))
    assert f["status"] == SC_OK
    f["Rt"] = np.concatenate([f["R"].ravel(), f["t"]]).astype(np.float32)
    return f


def _assert_same(got, exp, what=""):
    (gr, gl, gd, gn), (er, el, ed, en) = got, exp
    print(what, "rounds", None if gn is None else gn.tolist(), "expected", en.tolist(), "iters", gr["iters"][:8].tolist(), er["iters"][:8].tolist(),
          "stop", gr["stop"][:8].tolist(), er["stop"][:8].tolist(), "score", gr["score"][:8].tolist(), er["score"][:8].tolist())
    if gn is not None:
        assert gn.tolist() == en.tolist(), what
    assert np.array_equal(gl, el), what
    if gd is not None:
        assert gd.view(np.uint32).tobytes() == ed.view(np.uint32).tobytes(), what
    assert gr.tobytes() == er.tobytes(), what


def _device(pkg, r, sp, pose_bytes, stride, k, n, sel=None, want_d2=True, want_rounds=True):
    """the device form on host data: copies in, one call, one device-wide wait -> (records, label, d2 or None, rounds or None);
    every output is pre-filled with sentinel bytes"""
    import torch
    d_pose = torch.from_numpy(np.frombuffer(pose_bytes, np.uint8).copy()).cuda()
    d_sel = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).cuda()
    d_pol = torch.full((k * REC,), 0xAB, dtype=torch.uint8, device="cuda")
    d_label = torch.full((n,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
    d_d2 = torch.full((n,), 7.0, dtype=torch.float32, device="cuda") if want_d2 else None
    d_rounds = torch.full((2,), 0x5C5C5C5C, dtype=torch.int32, device="cuda") if want_rounds else None
    torch.cuda.synchronize()
    r.settle_poses_frame_device(sp, d_pose.data_ptr(), stride, k, 0 if d_sel is None else d_sel.data_ptr(), d_pol.data_ptr(),
                                d_label.data_ptr(), 0 if d_d2 is None else d_d2.data_ptr(), 0 if d_rounds is None else d_rounds.data_ptr())
    torch.cuda.synchronize()
    assert d_pose.cpu().numpy().tobytes() == pose_bytes  # d_pose is read, never written
    return (np.frombuffer(d_pol.cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE), d_label.cpu().numpy(),
            None if d_d2 is None else d_d2.cpu().numpy(), None if d_rounds is None else d_rounds.cpu().numpy().view(np.uint32))


def _small_lists(sc, n):
    gt = SR.rt_of(sc.R_gt, sc.t_gt)
    two = SR.perturbed(gt, 2, 100 + n, 1e-2, 2e-2)
    return {1: two[:1], 2: two, 4: np.stack([two[0], two[1], SR.far(gt), two[0]])}


# ---- the reference: every size, every pose count, max_iter 1, 2 and 16 ---------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 129])
def test_small_frames_equal_the_reference(pkg, O, reg, n):
    sc = SR.scene(pkg, n)
    _frame(pkg, reg, sc.src, sc.tgt)
    for K, poses in _small_lists(sc, n).items():
        for max_iter in (1, 2, 16):
            exp = SR.settle(O, sc.src, sc.tgt, poses, SR.TAU, max_iter=max_iter)
            got = reg.settle_poses_frame(poses, max_iter=max_iter)
            _assert_same(got, exp, f"n={n} K={K} max_iter={max_iter}")
            assert int(got[0]["score"].sum()) == int((got[1] >= 0).sum())  # the inlier-count mode
        dev = _device(pkg, reg, pkg.make_settle_params(), poses.tobytes(), 48, K, n)
        _assert_same(dev, exp, f"n={n} K={K} device form")


@pytest.mark.parametrize("name,iters", [("gt", (16,)), ("perturbed", (1, 2, 16)), ("far_dup", (16,)), ("many8", (1, 2, 16)), ("many64", (2,))])
def test_the_two_motion_scene_equals_the_reference(pkg, O, reg, name, iters):
    """K = 2, 4 (a far pose and a duplicate), 8 (K x 24 chunks x 9 entries exceed the 1024 lanes: a second trip of the deal), 64;
    max_iter 1 and 2 end in SC_POLISH_STOP_MAX_ITER and take the extra labelling pass"""
    mo = SR.motions(pkg)
    n = len(mo.src)
    poses = SR.starts(pkg)[name]
    K = len(poses)
    _frame(pkg, reg, mo.src, mo.tgt)
    for max_iter in iters:
        exp = SR.settle(O, mo.src, mo.tgt, poses, SR.TAU, max_iter=max_iter)
        got = reg.settle_poses_frame(poses, max_iter=max_iter)
        _assert_same(got, exp, f"{name} max_iter={max_iter}")
        if max_iter < 16:
            assert got[3].tolist() == [max_iter, SR.STOP_MAX_ITER]
    # host form == device form, with and without d_d2 / d_rounds; the call may be repeated
    sp = pkg.make_settle_params(max_iter=iters[-1])
    _assert_same(_device(pkg, reg, sp, poses.tobytes(), 48, K, n), exp, f"{name} device form")
    bare = _device(pkg, reg, sp, poses.tobytes(), 48, K, n, want_d2=False, want_rounds=False)
    assert bare[2] is None and bare[3] is None and np.array_equal(bare[1], exp[1]) and bare[0].tobytes() == exp[0].tobytes()
    host_bare = reg.settle_poses_frame(poses, max_iter=iters[-1], want_d2=False, want_rounds=False)
    assert host_bare[0].tobytes() == exp[0].tobytes() and np.array_equal(host_bare[1], exp[1])


# ---- the selection, the score modes, the strides and the statuses --------------------------------------------------------------------
def test_the_byte_mask_and_the_score_modes(pkg, O, reg):
    mo = SR.motions(pkg)
    n = len(mo.src)
    poses = SR.starts(pkg)["far_dup"]
    _frame(pkg, reg, mo.src, mo.tgt)
    sel = (np.arange(n) % 3 != 0).astype(np.uint8) * 5  # (any non-zero byte)
    exp = SR.settle(O, mo.src, mo.tgt, poses, SR.TAU, part=sel)
    got = reg.settle_poses_frame(poses, sel_mode=pkg.SC_ASSIGN_SEL_MASK, sel=sel)
    _assert_same(got, exp, "mask")
    assert (got[1][sel == 0] == -1).all() and (got[2][sel == 0].view(np.uint32) == 0x7F800000).all() and (got[1][sel != 0] >= 0).sum() > 200
    _assert_same(_device(pkg, reg, pkg.make_settle_params(sel_mode=pkg.SC_ASSIGN_SEL_MASK), poses.tobytes(), 48, 4, n, sel), exp, "mask, device")
    # with SEL_NONE a selection that is given is not read
    plain = SR.settle(O, mo.src, mo.tgt, poses, SR.TAU)
    _assert_same(reg.settle_poses_frame(poses, sel=np.zeros(n, np.uint8)), plain, "a selection that is not read")
    for score_mode in (1, 2):
        _frame(pkg, reg, mo.src, mo.tgt, score_mode=score_mode)
        exp = SR.settle(O, mo.src, mo.tgt, poses, SR.TAU, score_mode=score_mode)
        got = reg.settle_poses_frame(poses)
        _assert_same(got, exp, f"score_mode {score_mode}")
        assert got[0].tobytes() != plain[0].tobytes() and got[0]["Rt"].tobytes() == plain[0]["Rt"].tobytes()  # only the tallies differ


def test_strides_and_statuses(pkg, O, reg):
    mo = SR.motions(pkg)
    n = len(mo.src)
    two = SR.starts(pkg)["perturbed"]
    _frame(pkg, reg, mo.src, mo.tgt)
    good = reg.settle_poses_frame(two)
    _assert_same(good, SR.settle(O, mo.src, mo.tgt, two, SR.TAU), "stride 48")
    for dt in (pkg.api.POLISH_BATCH_RESULT_DTYPE, pkg.BATCH_RESULT_DTYPE):  # stride 64 and stride 80, with the flag
        pose = np.zeros(5, dt)
        pose["Rt"] = [two[0], two[0], two[1], two[1], two[1]]
        pose["status"] = [SC_ENOHYP, SC_OK, 77, SC_OK, SC_OK]  # a plane of SC_ENOHYP, a foreign status ...
        pose["Rt"][4][7] = np.nan                              # ... and a NaN pose among live ones
        exp = SR.settle(O, mo.src, mo.tgt, pose["Rt"], SR.TAU, statuses=pose["status"])
        got = reg.settle_poses_frame(pose, flags=pkg.SC_SETTLE_STATUS)
        _assert_same(got, exp, f"stride {dt.itemsize}, the flag")
        assert got[0]["status"].tolist() == [SC_ENOHYP, SC_OK, 77, SC_OK, SC_EINVAL]
        assert got[0][[1, 3]].tobytes() == good[0].tobytes() and np.array_equal(np.where(got[1] == 1, 0, np.where(got[1] == 3, 1, got[1])), good[1])
        _assert_same(_device(pkg, reg, pkg.make_settle_params(flags=pkg.SC_SETTLE_STATUS), pose.tobytes(), dt.itemsize, 5, n), exp, "device")
        # without the flag byte 48 is not read: poses 0 and 2 are poses like any other
        plain = reg.settle_poses_frame(pose)
        _assert_same(plain, SR.settle(O, mo.src, mo.tgt, pose["Rt"], SR.TAU), f"stride {dt.itemsize}, no flag")
        assert plain[0]["status"].tolist() == [SC_OK, SC_OK, SC_OK, SC_OK, SC_EINVAL]


# ---- the equalities of the header, GPU against GPU ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,max_iter", [("far_dup", 16), ("many8", 2)])
def test_the_composed_loop_of_the_existing_entries_gives_the_same(pkg, O, reg, name, max_iter):
    """equality 1: R rounds of sc_assign_poses_frame_device(BEST) + sc_polish_poses_device(SEL_LABEL, max_iter 1, STATUS), enqueued back
    to back, end in the same Rt; a last sc_assign_poses_frame_device writes d_label, d_d2 and every score"""
    import torch
    mo = SR.motions(pkg)
    n = len(mo.src)
    poses = SR.starts(pkg)[name]
    K = len(poses)
    _frame(pkg, reg, mo.src, mo.tgt)
    rec, lab, d2, rounds = reg.settle_poses_frame(poses, max_iter=max_iter)
    R = int(rounds[0]) + (1 if rounds[1] == SR.STOP_FIXED else 0)
    d_pol = [torch.from_numpy(poses.copy()).cuda().view(torch.uint8), torch.zeros(K * REC, dtype=torch.uint8, device="cuda"),
             torch.zeros(K * REC, dtype=torch.uint8, device="cuda")]
    d_label = torch.zeros(n, dtype=torch.int32, device="cuda"); d_d2 = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_asg = torch.zeros(K * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    PP, AP = pkg.make_polish_poses_params, pkg.make_assign_params
    cur, stride, flag = 0, 48, 0
    for i in range(R):
        nxt = 1 + i % 2
        reg.assign_poses_frame_device(AP(flags=flag), d_pol[cur].data_ptr(), stride, K, 0, d_label.data_ptr(), 0, d_asg.data_ptr())
        reg.polish_poses_device(PP(max_iter=1, sel_mode=pkg.SC_POLISH_POSES_SEL_LABEL, flags=flag), d_pol[cur].data_ptr(), stride, K,
                                d_label.data_ptr(), d_pol[nxt].data_ptr(), 0)
        cur, stride, flag = nxt, 64, 1
    reg.assign_poses_frame_device(AP(flags=flag), d_pol[cur].data_ptr(), stride, K, 0, d_label.data_ptr(), d_d2.data_ptr(), d_asg.data_ptr())
    torch.cuda.synchronize()
    pol = np.frombuffer(d_pol[cur].cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE)
    asg = np.frombuffer(d_asg.cpu().numpy().tobytes(), pkg.ASSIGN_RESULT_DTYPE)
    print(name, "rounds", rounds.tolist(), "composed rounds", R, asg["count"].tolist())
    assert R >= 2 and pol["Rt"].tobytes() == rec["Rt"].tobytes()
    assert np.array_equal(d_label.cpu().numpy(), lab) and d_d2.cpu().numpy().tobytes() == d2.tobytes()
    assert np.array_equal(asg["score"], rec["score"]) and np.array_equal(asg["count"], np.bincount(lab[lab >= 0], minlength=K))


def test_one_pose_is_polish_poses_and_a_settled_list_stays(pkg, O, reg):
    mo = SR.motions(pkg)
    S = SR.starts(pkg)
    _frame(pkg, reg, mo.src, mo.tgt)
    # equality 2
    for max_iter in (1, 2, 16):
        rec, lab, d2, rounds = reg.settle_poses_frame(S["perturbed"][:1], max_iter=max_iter)
        pol, mask = reg.polish_poses(S["perturbed"][:1], max_iter=max_iter)
        print(max_iter, rounds.tolist(), rec["iters"].tolist(), pol["iters"].tolist(), rec["stop"].tolist(), pol["stop"].tolist())
        assert rec.tobytes() == pol.tobytes() and np.array_equal(lab, mask[0].astype(np.int32) - 1), max_iter
    far = reg.settle_poses_frame(SR.far(S["gt"][0]))  # a pose without members: declined at once, nothing counted
    assert far[3].tolist() == [0, SR.STOP_FIXED] and far[0]["stop"].tolist() == [SR.STOP_DECLINED] and (far[1] == -1).all()
    assert far[0].tobytes() == reg.polish_poses(SR.far(S["gt"][0]))[0].tobytes()
    # equality 4
    rec, lab, d2, rounds = reg.settle_poses_frame(S["far_dup"])
    assert rounds[1] == SR.STOP_FIXED and rounds[0] >= 2
    again = reg.settle_poses_frame(rec, flags=pkg.SC_SETTLE_STATUS)
    assert again[3].tolist() == [0, SR.STOP_FIXED] and again[0]["Rt"].tobytes() == rec["Rt"].tobytes()
    assert np.array_equal(again[1], lab) and again[2].tobytes() == d2.tobytes() and not again[0]["iters"].any()
    assert np.array_equal(again[0]["score"], rec["score"]) and np.array_equal(again[0]["score0"], rec["score"])
    assert again[0]["stop"].tolist() == rec["stop"].tolist()


# ---- the frame is untouched ------------------------------------------------------------------------------------------------------------
def test_the_frame_still_peels_and_the_neighbours_still_answer(pkg, O):
    mo = SR.motions(pkg)
    poses = SR.starts(pkg)["perturbed"]
    with_call, without = pkg.Registrar(0), pkg.Registrar(0)
    try:
        _frame(pkg, with_call, mo.src, mo.tgt)
        _frame(pkg, without, mo.src, mo.tgt)
        exp = SR.settle(O, mo.src, mo.tgt, poses, SR.TAU)
        _assert_same(with_call.settle_poses_frame(poses), exp, "before the round")
        a, b = with_call.peel(), without.peel()
        assert a["status"] == b["status"] == SC_OK and np.array_equal(a["mask"], b["mask"]) and a["R"].tobytes() == b["R"].tobytes()
        _assert_same(with_call.settle_poses_frame(poses), exp, "between the rounds")
        pa, pb = with_call.polish_poses(poses), without.polish_poses(poses)  # (they share the chunk scratch)
        assert pa[0].tobytes() == pb[0].tobytes() and np.array_equal(pa[1], pb[1])
        assert with_call.pose_info_frame(poses).tobytes() == without.pose_info_frame(poses).tobytes()
        aa, ab = with_call.assign_poses_frame(poses), without.assign_poses_frame(poses)
        assert np.array_equal(aa[0], ab[0]) and aa[2].tobytes() == ab[2].tobytes()
        a, b = with_call.peel(), without.peel()
        assert a["status"] == b["status"] and np.array_equal(a["mask"], b["mask"])
        _assert_same(with_call.settle_poses_frame(poses), exp, "after everything")
    finally:
        with_call.close(); without.close()


# ---- what is refused, and what a refused call leaves -----------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_frame(pkg, O):
    L = pkg.load_library()
    sc = SR.scene(pkg, 129)
    r = pkg.Registrar(0)
    try:
        pose = np.zeros(2, pkg.BATCH_RESULT_DTYPE)
        pol = np.zeros(2, pkg.api.POLISH_BATCH_RESULT_DTYPE); label = np.zeros(129, np.int32); d2 = np.zeros(129, np.float32)
        rounds = np.zeros(2, np.uint32)
        sel = np.ones(129, np.uint8)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

        def call(sp, stride=80, k=2, sel=None, pose=pose, pol=pol, label=label, entry=L.sc_settle_poses_frame):
            rc = entry(r._h, None if sp is None else C.byref(sp), vp(pose), stride, k, vp(sel), vp(pol), vp(label), vp(d2), vp(rounds))
            return rc, L.sc_last_error(r._h).decode()

        ok = pkg.make_settle_params()
        rc, text = call(ok)  # no frame on a fresh context
        assert rc == SC_EINVAL and "no frame" in text and "sc_settle_poses_frame" in text
        f = _frame(pkg, r, sc.src, sc.tgt)
        pose["Rt"], pose["status"] = f["Rt"], SC_OK
        good = r.settle_poses_frame(pose)
        _assert_same(good, SR.settle(O, sc.src, sc.tgt, pose["Rt"], SR.TAU), "good")
        short = pkg.make_settle_params(); short.size = 28
        res = pkg.make_settle_params(); res.reserved[3] = 1
        mk = pkg.make_settle_params
        cases = {
            "sp NULL": (lambda: call(None), "NULL"),
            "pose NULL": (lambda: call(ok, pose=None), "NULL"),
            "pol NULL": (lambda: call(ok, pol=None), "NULL"),
            "label NULL": (lambda: call(ok, label=None), "NULL"),
            "size": (lambda: call(short), "size"),
            "max_iter 0": (lambda: call(mk(max_iter=0)), "max_iter"),
            "max_iter 65": (lambda: call(mk(max_iter=65)), "max_iter"),
            "sel_mode 2": (lambda: call(mk(sel_mode=2), sel=sel), "sel_mode"),
            "mask without sel": (lambda: call(mk(sel_mode=1)), "sel is NULL"),
            "flag 2": (lambda: call(mk(flags=2)), "flag"),
            "reserved": (lambda: call(res), "reserved"),
            "n_poses 0": (lambda: call(ok, k=0), "n_poses"),
            "n_poses 65": (lambda: call(ok, k=65), "n_poses"),
            "stride 0": (lambda: call(ok, stride=0), "pose_stride"),
            "stride 44": (lambda: call(ok, stride=44), "pose_stride"),
            "stride 50": (lambda: call(ok, stride=50), "pose_stride"),
            "stride 48 with the flag": (lambda: call(mk(flags=1), stride=48), "pose_stride"),
            "device form, stride 50": (lambda: call(ok, stride=50, entry=L.sc_settle_poses_frame_device), "sc_settle_poses_frame_device"),
        }
        for what, (fn, word) in cases.items():
            rc, text = fn()
            print(what, rc, text)
            assert rc == SC_EINVAL and word in text and "sc_settle_poses_frame" in text, what
        _assert_same(r.settle_poses_frame(pose), good, "the refused calls left the context and the frame")
        assert r.peel()["status"] in (SC_OK, SC_ENOHYP)
        assert call(mk(sel_mode=1), sel=sel)[0] == SC_OK
        # a batch entry ends the frame
        s2, t2 = batch_ref.scene(pkg, 128, .3)
        r.register_batch_raw(s2, t2, np.array([0, 128], np.uint32), _params(pkg))
        rc, text = call(ok)
        assert rc == SC_EINVAL and "no frame" in text
        # a call outstanding on the context: refused, host and device form; after sc_wait the frame it left answers as before
        import torch
        ds, dt = torch.from_numpy(sc.src).cuda(), torch.from_numpy(sc.tgt).cuda()
        d_Rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_mask = torch.zeros(129, dtype=torch.uint8, device="cuda")
        r.register_device_async(ds.data_ptr(), dt.data_ptr(), 129, _params(pkg), d_Rt.data_ptr(), d_mask.data_ptr())
        for entry in (L.sc_settle_poses_frame, L.sc_settle_poses_frame_device):
            rc, text = call(ok, entry=entry)
            assert rc == SC_EINVAL and "outstanding" in text
        assert r.wait()[0] == SC_OK
        r._frame_n = 129
        _assert_same(r.settle_poses_frame(pose), good, "after the async frame")  # no output depends on how the frame was enqueued
    finally:
        r.close()
