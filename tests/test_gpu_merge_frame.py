"""GPU: duplicate poses found and folded on a scored frame (include/saccot.h, sc_merge_poses_frame / sc_merge_poses_frame_device).

The expected value of every case is tests/merge_ref.py — the support sets from the canonical residual's bits, the overlap table, the
strength order and the greedy fold, all integers — and every comparison is bit for bit: the 64 bytes of every record, every parent,
every cell of the overlap table, both count words.  No tolerances.  The equalities the header promises are checked GPU against GPU
as well: sc_polish_poses_device's score0, the kept list fed in again, and the closed loop into sc_settle_poses_frame_device.
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref
import merge_ref as MR
import settle_ref as SR

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
REC = 64
TILE = 512       # correspondences of one workgroup of the support launch (MERGE_TILE, sc_merge.hpp)
PAIR_TILE = 32   # poses a side of one workgroup of the overlap launch (MERGE_PAIR_TILE)
FRACTIONS = ((1, 1), (1, 2), (1, 8))


def _params(pkg, **kw):
    return pkg.make_params(**MR.kw_of(), **kw)


def _frame(pkg, r, src, tgt, **kw):
    """sc_register on (src, tgt): the frame the context then holds -> its result, Rt (12,) with it"""
    f = r.register(src, tgt, params=_params(pkg, **kw))
    assert f["status"] == SC_OK
    f["Rt"] = np.concatenate([f["R"].ravel(), f["t"]]).astype(np.float32)
    return f


def _assert_same(got, exp, what=""):
    (gr, gp, gx, gc), (er, ep, ex, ec) = got, exp
    print(what, "count", None if gc is None else gc.tolist(), "expected", ec.tolist(), "parent", gp[:12].tolist(), ep[:12].tolist(),
          "counts", gr["count"][:12].tolist(), er["count"][:12].tolist(), "scores", gr["score"][:12].tolist(), er["score"][:12].tolist())
    if gc is not None:
        assert gc.tolist() == ec.tolist(), what
    assert np.array_equal(gp, ep), what
    if gx is not None:
        assert gx.shape == ex.shape and np.array_equal(gx, ex), what
    assert gr.tobytes() == er.tobytes(), what


def _device(pkg, r, mp, pose_bytes, stride, k, sel=None, want_overlap=True, want_count=True):
    """the device form on host data: copies in, one call, one device-wide wait -> (records, parent, overlap or None, count or None);
    every output is pre-filled with sentinel bytes"""
    import torch
    d_pose = torch.from_numpy(np.frombuffer(pose_bytes, np.uint8).copy()).cuda()
    d_sel = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).cuda()
    d_out = torch.full((k * REC,), 0xAB, dtype=torch.uint8, device="cuda")
    d_parent = torch.full((k,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
    d_overlap = torch.full((k * k,), 0x3C3C3C3C, dtype=torch.int32, device="cuda") if want_overlap else None
    d_count = torch.full((2,), 0x5C5C5C5C, dtype=torch.int32, device="cuda") if want_count else None
    torch.cuda.synchronize()
    r.merge_poses_frame_device(mp, d_pose.data_ptr(), stride, k, 0 if d_sel is None else d_sel.data_ptr(), d_out.data_ptr(),
                               d_parent.data_ptr(), 0 if d_overlap is None else d_overlap.data_ptr(), 0 if d_count is None else d_count.data_ptr())
    torch.cuda.synchronize()
    assert d_pose.cpu().numpy().tobytes() == pose_bytes  # d_pose is read, never written
    return (np.frombuffer(d_out.cpu().numpy().tobytes(), pkg.MERGE_POSE_DTYPE), d_parent.cpu().numpy(),
            None if d_overlap is None else d_overlap.cpu().numpy().view(np.uint32).reshape(k, k),
            None if d_count is None else d_count.cpu().numpy().view(np.uint32))


def _list_of(sc, K, seed):
    """K poses around the scene's motion: neighbours, from K = 4 on a far pose and an exact copy, from K = 8 on MR.many's"""
    gt = MR.rt_of(sc.R_gt, sc.t_gt)
    if K >= 8:
        return MR.many(gt, K, seed)
    two = MR.perturbed(gt, 2, seed, 1e-2, 2e-2)
    return {1: two[:1], 2: two, 4: np.stack([two[0], two[1], MR.far(gt), two[0]])}[K]


# ---- the reference: the word boundaries, the tile boundaries, every pose count -------------------------------------------------------
@pytest.mark.parametrize("n", [65, 129, TILE + 1, 2 * TILE + 1])
def test_small_frames_equal_the_reference(pkg, O, reg, n):
    """n = 65, 129: the last ballot word is partial; TILE + 1, 2 TILE + 1: a second and a third workgroup that own one
    correspondence.  K = 33: one pose past the overlap launch's pair tile (three tiles, one of them off the diagonal)."""
    sc = MR.scene(pkg, n)
    _frame(pkg, reg, sc.src, sc.tgt)
    for K in (1, 2, 4, 8, PAIR_TILE + 1, 64):
        poses = _list_of(sc, K, 100 + n + K)
        exp = MR.merge(O, sc.src, sc.tgt, poses, MR.TAU)
        _assert_same(reg.merge_poses_frame(poses), exp, f"n={n} K={K}")
        if K in (2, PAIR_TILE + 1):
            tight = MR.merge(O, sc.src, sc.tgt, poses, MR.TAU, measure=MR.OVER_UNION, num=1, den=1)
            _assert_same(_device(pkg, reg, pkg.make_merge_params(measure=1, num=1, den=1), poses.tobytes(), 48, K), tight, f"n={n} K={K} device form")
    assert exp[3][1] == 64 and exp[3][0] < 64 and (exp[1][exp[1] >= 0] != np.flatnonzero(exp[1] >= 0)).any()  # K = 64 folds something


def test_a_thousand_poses(pkg, O, reg):
    """K = SC_MERGE_MAX_POSES: sixteen rounds of the decide launch, 528 tiles of the overlap launch, 56 KB of poses in LDS"""
    sc = MR.scene(pkg, 129)
    _frame(pkg, reg, sc.src, sc.tgt)
    poses = MR.many(MR.rt_of(sc.R_gt, sc.t_gt), 1024, 77)
    poses[1000] = poses[18]
    exp = MR.merge(O, sc.src, sc.tgt, poses, MR.TAU, num=3, den=4)
    got = reg.merge_poses_frame(poses, num=3, den=4)
    _assert_same(got, exp, "K=1024")
    assert 2 <= got[3][0] < 1024 and got[3][1] == 1024 and got[1][1000] == got[1][18] != 1000
    packed = _device(pkg, reg, pkg.make_merge_params(num=3, den=4, flags=pkg.SC_MERGE_COMPACT), poses.tobytes(), 48, 1024, want_overlap=False)
    _assert_same(packed, MR.merge(O, sc.src, sc.tgt, poses, MR.TAU, num=3, den=4, compact=True), "K=1024, compact, no table")


# ---- the two-motion scene: every list, both measures, three fractions, min_count ----------------------------------------------------
@pytest.mark.parametrize("name", ["dup", "near", "nested", "invalid", "starved", "many64"])
def test_the_two_motion_scene_equals_the_reference(pkg, O, reg, name):
    mo = MR.motions(pkg)
    poses = MR.lists(pkg)[name]
    K = len(poses)
    _frame(pkg, reg, mo.src, mo.tgt)
    for measure in (MR.OVER_MIN, MR.OVER_UNION):
        for num, den in FRACTIONS:
            for min_count in (0, 7):
                rule = dict(measure=measure, num=num, den=den, min_count=min_count)
                exp = MR.merge(O, mo.src, mo.tgt, poses, MR.TAU, **rule)
                _assert_same(reg.merge_poses_frame(poses, **rule), exp, f"{name} {rule}")
    # host form == device form, with and without d_overlap / d_count, compact or not; the call may be repeated
    for compact in (False, True):
        mp = pkg.make_merge_params(min_count=7, flags=pkg.SC_MERGE_COMPACT if compact else 0)
        exp = MR.merge(O, mo.src, mo.tgt, poses, MR.TAU, min_count=7, compact=compact)
        first = _device(pkg, reg, mp, poses.tobytes(), 48, K)
        _assert_same(first, exp, f"{name} device form, compact {compact}")
        again = _device(pkg, reg, mp, poses.tobytes(), 48, K)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
        bare = _device(pkg, reg, mp, poses.tobytes(), 48, K, want_overlap=False, want_count=False)
        assert bare[2] is None and bare[3] is None and np.array_equal(bare[1], exp[1]) and bare[0].tobytes() == exp[0].tobytes()
        host_bare = reg.merge_poses_frame(poses, mp, want_overlap=False, want_count=False)
        assert host_bare[0].tobytes() == exp[0].tobytes() and np.array_equal(host_bare[1], exp[1])
        if compact:
            kept = int(exp[3][0])
            assert (first[0]["status"][:kept] == SC_OK).all() and (first[0]["status"][kept:] != SC_OK).all()
            assert (np.diff(first[0]["index"][:kept]) > 0).all() if kept > 1 else True


def test_the_byte_mask_and_the_score_modes(pkg, O, reg):
    mo = MR.motions(pkg)
    n = len(mo.src)
    poses = MR.lists(pkg)["dup"]
    _frame(pkg, reg, mo.src, mo.tgt)
    sel = (np.arange(n) % 3 != 0).astype(np.uint8) * 5  # (any non-zero byte)
    exp = MR.merge(O, mo.src, mo.tgt, poses, MR.TAU, part=sel)
    got = reg.merge_poses_frame(poses, sel_mode=pkg.SC_ASSIGN_SEL_MASK, sel=sel)
    _assert_same(got, exp, "mask")
    plain = MR.merge(O, mo.src, mo.tgt, poses, MR.TAU)
    assert 0 < got[0]["count"][6] < plain[0]["count"][6]
    _assert_same(_device(pkg, reg, pkg.make_merge_params(sel_mode=pkg.SC_ASSIGN_SEL_MASK), poses.tobytes(), 48, 8, sel), exp, "mask, device")
    _assert_same(reg.merge_poses_frame(poses, sel=np.zeros(n, np.uint8)), plain, "a selection that is not read")  # SEL_NONE
    for score_mode in (1, 2):
        _frame(pkg, reg, mo.src, mo.tgt, score_mode=score_mode)
        for name in ("dup", "near"):
            exp = MR.merge(O, mo.src, mo.tgt, MR.lists(pkg)[name], MR.TAU, score_mode=score_mode)
            got = reg.merge_poses_frame(MR.lists(pkg)[name])
            _assert_same(got, exp, f"{name}, score_mode {score_mode}")
        assert not np.array_equal(got[0]["score"], got[0]["count"])  # the strength is the score, not the count


def test_strides_and_statuses(pkg, O, reg):
    mo = MR.motions(pkg)
    L = MR.lists(pkg)
    _frame(pkg, reg, mo.src, mo.tgt)
    a, b = L["near"][4], L["near"][7]
    for dt in (pkg.MERGE_POSE_DTYPE, pkg.BATCH_RESULT_DTYPE):  # stride 64 and stride 80
        pose = np.zeros(6, dt)
        pose["Rt"] = [a, a, b, b, b, L["near"][0]]
        pose["status"] = [SC_ENOHYP, SC_OK, 77, SC_OK, SC_OK, SC_OK]  # a plane of SC_ENOHYP, a foreign status ...
        pose["Rt"][4][7] = np.nan                                      # ... and a NaN pose among live ones
        for compact in (0, pkg.SC_MERGE_COMPACT):
            exp = MR.merge(O, mo.src, mo.tgt, pose["Rt"], MR.TAU, statuses=pose["status"], compact=bool(compact))
            got = reg.merge_poses_frame(pose, flags=pkg.SC_MERGE_STATUS | compact)
            _assert_same(got, exp, f"stride {dt.itemsize}, the flag, compact {compact}")
            _assert_same(_device(pkg, reg, pkg.make_merge_params(flags=pkg.SC_MERGE_STATUS | compact), pose.tobytes(), dt.itemsize, 6), exp, "device")
        assert got[1].tolist() == [-1, 1, -1, 3, -1, 1] and got[3].tolist() == [2, 3]
        assert sorted(got[0]["status"].tolist()) == sorted([SC_ENOHYP, SC_OK, 77, SC_OK, SC_EINVAL, SC_ENOHYP])
        # without the flag byte 48 is not read: poses 0 and 2 are poses like any other, and copies
        plain = reg.merge_poses_frame(pose)
        _assert_same(plain, MR.merge(O, mo.src, mo.tgt, pose["Rt"], MR.TAU), f"stride {dt.itemsize}, no flag")
        assert plain[1].tolist() == [0, 0, 2, 2, -1, 0]
    _assert_same(reg.merge_poses_frame(pose["Rt"].copy()), MR.merge(O, mo.src, mo.tgt, pose["Rt"], MR.TAU), "stride 48")


# ---- the equalities of the header, GPU against GPU -----------------------------------------------------------------------------------
@pytest.mark.parametrize("score_mode", [0, 1, 2])
def test_the_score_is_polish_poses_score0(pkg, O, reg, score_mode):
    """equality 1, against sc_polish_poses_device under the same selection"""
    import torch
    mo = MR.motions(pkg)
    n = len(mo.src)
    _frame(pkg, reg, mo.src, mo.tgt, score_mode=score_mode)
    sel = (np.arange(n) % 4 != 1).astype(np.uint8)
    for name in ("dup", "invalid", "many64"):
        poses = MR.lists(pkg)[name]
        K = len(poses)
        for mask in (None, sel):
            d_pose = torch.from_numpy(poses.copy()).cuda()
            d_sel = None if mask is None else torch.from_numpy(mask).cuda()
            d_pol = torch.zeros(K * REC, dtype=torch.uint8, device="cuda")
            qp = pkg.make_polish_poses_params(max_iter=1, sel_mode=pkg.SC_POLISH_POSES_SEL_NONE if mask is None else pkg.SC_POLISH_POSES_SEL_MASK)
            reg.polish_poses_device(qp, d_pose.data_ptr(), 48, K, 0 if d_sel is None else d_sel.data_ptr(), d_pol.data_ptr(), 0)
            torch.cuda.synchronize()
            pol = np.frombuffer(d_pol.cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE)
            mp = pkg.make_merge_params(sel_mode=pkg.SC_ASSIGN_SEL_NONE if mask is None else pkg.SC_ASSIGN_SEL_MASK)
            rec, parent, x, count = _device(pkg, reg, mp, poses.tobytes(), 48, K, mask)
            print(name, score_mode, rec["score"][:8].tolist(), pol["score0"][:8].tolist())
            assert np.array_equal(rec["score"], pol["score0"]) and np.array_equal(np.diag(x), rec["count"])
            if score_mode == 0:
                assert np.array_equal(rec["score"], rec["count"])


def test_the_kept_list_goes_in_again_and_a_copy_is_never_kept(pkg, O, reg):
    mo = MR.motions(pkg)
    _frame(pkg, reg, mo.src, mo.tgt)
    # equality 3
    for name in ("dup", "near", "starved", "invalid", "many64"):
        for flags in (0, pkg.SC_MERGE_COMPACT):
            rec, parent, x, count = reg.merge_poses_frame(MR.lists(pkg)[name], flags=flags)
            again = reg.merge_poses_frame(rec, flags=flags | pkg.SC_MERGE_STATUS)
            kept = rec["status"] == SC_OK
            assert again[3][0] == count[0] == kept.sum() and again[0]["Rt"][kept].tobytes() == rec["Rt"][kept].tobytes(), name
            assert np.array_equal(again[0]["status"], rec["status"]) and np.array_equal(again[0]["count"][kept], rec["count"][kept]), name
            assert np.array_equal(again[0]["score"][kept], rec["score"][kept]), name
            if flags:  # the kept prefix alone, as a caller who waited passes it on
                head = reg.merge_poses_frame(rec[:int(count[0])], flags=flags | pkg.SC_MERGE_STATUS)
                assert head[3].tolist() == [count[0], count[0]] and head[0]["Rt"].tobytes() == rec["Rt"][:int(count[0])].tobytes(), name
    # equality 2
    for measure in (0, 1):
        for num, den in FRACTIONS + ((65536, 65536), (1, 65536)):
            parent = reg.merge_poses_frame(MR.lists(pkg)["many64"], measure=measure, num=num, den=den)[1]
            assert parent[5] == parent[1] != 5, (measure, num, den)
    # equality 5
    rec, parent, x, count = reg.merge_poses_frame(MR.lists(pkg)["nested"], num=1, den=1)
    assert parent.tolist() == [2, 1, 2] and x[0, 2] == rec["count"][0]


@pytest.mark.parametrize("name", ["dup", "near"])
def test_the_closed_loop_into_settle(pkg, O, reg, name):
    """the merge output, still on the device, into sc_settle_poses_frame_device at stride 64 with the status flag: what
    tests/settle_ref.py gives on the same records"""
    import torch
    mo = MR.motions(pkg)
    n = len(mo.src)
    poses = MR.lists(pkg)[name]
    K = len(poses)
    _frame(pkg, reg, mo.src, mo.tgt)
    d_pose = torch.from_numpy(poses.copy()).cuda()
    d_out = torch.zeros(K * REC, dtype=torch.uint8, device="cuda"); d_parent = torch.zeros(K, dtype=torch.int32, device="cuda")
    d_pol = torch.zeros(K * REC, dtype=torch.uint8, device="cuda"); d_label = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_rounds = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    reg.merge_poses_frame_device(pkg.make_merge_params(), d_pose.data_ptr(), 48, K, 0, d_out.data_ptr(), d_parent.data_ptr())
    reg.settle_poses_frame_device(pkg.make_settle_params(flags=pkg.SC_SETTLE_STATUS), d_out.data_ptr(), REC, K, 0, d_pol.data_ptr(),
                                  d_label.data_ptr(), 0, d_rounds.data_ptr())
    torch.cuda.synchronize()
    rec = np.frombuffer(d_out.cpu().numpy().tobytes(), pkg.MERGE_POSE_DTYPE)
    exp_rec = MR.merge(O, mo.src, mo.tgt, poses, MR.TAU)[0]
    assert rec.tobytes() == exp_rec.tobytes()
    exp = SR.settle(O, mo.src, mo.tgt, rec["Rt"], MR.TAU, statuses=rec["status"])
    pol = np.frombuffer(d_pol.cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE)
    print(name, "kept", (rec["status"] == SC_OK).sum(), "rounds", d_rounds.cpu().numpy().tolist(), exp[3].tolist(), "scores", pol["score"].tolist())
    assert pol.tobytes() == exp[0].tobytes() and np.array_equal(d_label.cpu().numpy(), exp[1]) and d_rounds.cpu().numpy().tolist() == exp[3].tolist()
    lab = d_label.cpu().numpy()
    assert set(np.unique(lab[lab >= 0]).tolist()) <= set(np.flatnonzero(rec["status"] == SC_OK).tolist())  # the dead records claim nothing
    assert (pol["score"][rec["status"] == SC_OK].astype(np.int64).sum()) == (lab >= 0).sum() > 500  # one strong edge per motion


# ---- the frame is untouched --------------------------------------------------------------------------------------------------------------
def test_the_frame_still_peels_and_the_neighbours_still_answer(pkg, O):
    mo = MR.motions(pkg)
    poses = MR.lists(pkg)["near"]
    with_call, without = pkg.Registrar(0), pkg.Registrar(0)
    try:
        _frame(pkg, with_call, mo.src, mo.tgt)
        _frame(pkg, without, mo.src, mo.tgt)
        exp = MR.merge(O, mo.src, mo.tgt, poses, MR.TAU)
        _assert_same(with_call.merge_poses_frame(poses), exp, "before the round")
        a, b = with_call.peel(), without.peel()
        assert a["status"] == b["status"] == SC_OK and np.array_equal(a["mask"], b["mask"]) and a["R"].tobytes() == b["R"].tobytes()
        _assert_same(with_call.merge_poses_frame(poses), exp, "between the rounds")
        pa, pb = with_call.polish_poses(poses), without.polish_poses(poses)
        assert pa[0].tobytes() == pb[0].tobytes() and np.array_equal(pa[1], pb[1])
        sa, sb = with_call.settle_poses_frame(poses[[4, 7]]), without.settle_poses_frame(poses[[4, 7]])
        assert sa[0].tobytes() == sb[0].tobytes() and np.array_equal(sa[1], sb[1])
        a, b = with_call.peel(), without.peel()
        assert a["status"] == b["status"] and np.array_equal(a["mask"], b["mask"])
        _assert_same(with_call.merge_poses_frame(poses), exp, "after everything")
    finally:
        with_call.close(); without.close()


# ---- what is refused, and what a refused call leaves -------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_frame(pkg, O):
    L = pkg.load_library()
    sc = MR.scene(pkg, 129)
    r = pkg.Registrar(0)
    try:
        pose = np.zeros(2, pkg.BATCH_RESULT_DTYPE)
        out = np.zeros(2, pkg.MERGE_POSE_DTYPE); parent = np.zeros(2, np.int32); overlap = np.zeros(4, np.uint32); count = np.zeros(2, np.uint32)
        sel = np.ones(129, np.uint8)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

        def call(mp, stride=80, k=2, sel=None, pose=pose, out=out, parent=parent, entry=L.sc_merge_poses_frame):
            rc = entry(r._h, None if mp is None else C.byref(mp), vp(pose), stride, k, vp(sel), vp(out), vp(parent), vp(overlap), vp(count))
            return rc, L.sc_last_error(r._h).decode()

        ok = pkg.make_merge_params()
        rc, text = call(ok)  # no frame on a fresh context
        assert rc == SC_EINVAL and "no frame" in text and "sc_merge_poses_frame" in text
        f = _frame(pkg, r, sc.src, sc.tgt)
        pose["Rt"], pose["status"] = f["Rt"], SC_OK
        good = r.merge_poses_frame(pose)
        _assert_same(good, MR.merge(O, sc.src, sc.tgt, pose["Rt"], MR.TAU), "good")
        assert good[1].tolist() == [0, 0]
        short = pkg.make_merge_params(); short.size = 28
        res = pkg.make_merge_params(); res.reserved[0] = 1
        mk = pkg.make_merge_params
        cases = {
            "mp NULL": (lambda: call(None), "NULL"),
            "pose NULL": (lambda: call(ok, pose=None), "NULL"),
            "out NULL": (lambda: call(ok, out=None), "NULL"),
            "parent NULL": (lambda: call(ok, parent=None), "NULL"),
            "size": (lambda: call(short), "size"),
            "measure 2": (lambda: call(mk(measure=2)), "measure"),
            "num 0": (lambda: call(mk(num=0)), "num"),
            "num above den": (lambda: call(mk(num=3, den=2)), "num"),
            "den 65537": (lambda: call(mk(den=65537)), "den"),
            "sel_mode 2": (lambda: call(mk(sel_mode=2), sel=sel), "sel_mode"),
            "mask without sel": (lambda: call(mk(sel_mode=1)), "sel is NULL"),
            "flag 4": (lambda: call(mk(flags=4)), "flag"),
            "reserved": (lambda: call(res), "reserved"),
            "n_poses 0": (lambda: call(ok, k=0), "n_poses"),
            "n_poses 1025": (lambda: call(ok, k=1025), "n_poses"),
            "stride 0": (lambda: call(ok, stride=0), "pose_stride"),
            "stride 44": (lambda: call(ok, stride=44), "pose_stride"),
            "stride 50": (lambda: call(ok, stride=50), "pose_stride"),
            "stride 48 with the flag": (lambda: call(mk(flags=1), stride=48), "pose_stride"),
            "device form, stride 50": (lambda: call(ok, stride=50, entry=L.sc_merge_poses_frame_device), "sc_merge_poses_frame_device"),
        }
        for what, (fn, word) in cases.items():
            rc, text = fn()
            print(what, rc, text)
            assert rc == SC_EINVAL and word in text and "sc_merge_poses_frame" in text, what
        _assert_same(r.merge_poses_frame(pose), good, "the refused calls left the context and the frame")
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
        for entry in (L.sc_merge_poses_frame, L.sc_merge_poses_frame_device):
            rc, text = call(ok, entry=entry)
            assert rc == SC_EINVAL and "outstanding" in text
        assert r.wait()[0] == SC_OK
        r._frame_n = 129
        _assert_same(r.merge_poses_frame(pose), good, "after the async frame")  # no output depends on how the frame was enqueued
    finally:
        r.close()
