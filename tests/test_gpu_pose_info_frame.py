"""GPU: the fp64 information matrix on a scored frame (include/saccot.h, sc_pose_info_frame / sc_pose_info_frame_device).

The expected value of every case is tests/pose_info_frame_ref.py — tests/pose_info_ref.py's Python loops over numpy float64 scalars in
the contract's order, with the selection ANDed into the CPU restatement's mask — and every comparison is bit for bit: the 320 bytes of
every record (`tobytes`).  No tolerances.  Where sc_pose_info_batch can see the same problem (n <= 512) the two kernels are compared
with each other as well.  The scenes are checked on the CPU by tests/test_pose_info_frame_abi.py.
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref
import pose_info_frame_ref as PF

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOMEM, SC_ENOHYP = 0, -1, -2, -5
REC = 320
STAT_KEYS = ("n", "edges", "tri_total", "tri_kept", "tri_scored", "best_rank", "best_count")


def _params(pkg, soa=False, **kw):
    return pkg.make_params(**PF.kw_of(), layout=pkg.SC_SOA if soa else pkg.SC_AOS, **kw)


def _frame(pkg, r, src, tgt, soa=False, **kw):
    """sc_register on (src, tgt): the frame the context then holds -> its result, Rt (12,) with it"""
    a, b = (np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)) if soa else (src, tgt)
    f = r.register(a, b, params=_params(pkg, soa, **kw))
    assert f["status"] == SC_OK
    f["Rt"] = np.concatenate([f["R"].ravel(), f["t"]]).astype(np.float32)
    return f


def _records(pkg, t):
    return np.frombuffer(t.cpu().numpy().tobytes(), pkg.POSE_INFO_RESULT_DTYPE)


def _assert_info(got, exp, what=""):
    assert len(got) == len(exp), what
    for k in range(len(got)):
        print(what, k, int(got[k]["status"]), int(got[k]["inliers"]), float(got[k]["sse"]), "| expected", int(exp[k]["status"]),
              int(exp[k]["inliers"]), float(exp[k]["sse"]))
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


def _zero(status):
    z = np.zeros((), PF.RESULT_DTYPE); z["status"] = status
    return z.tobytes()


def _device(pkg, r, ip, pose_bytes, stride, k, sel=None):
    """the device form on host data: copies in, one call, one device-wide wait -> records (k,)"""
    import torch
    d_pose = torch.from_numpy(np.frombuffer(pose_bytes, np.uint8).copy()).cuda()
    d_sel = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel)).cuda()
    d_info = torch.full((k * REC,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.pose_info_frame_device(ip, d_pose.data_ptr(), stride, k, 0 if d_sel is None else d_sel.data_ptr(), d_info.data_ptr())
    torch.cuda.synchronize()
    assert d_pose.cpu().numpy().tobytes() == pose_bytes  # d_pose is read, never written
    return _records(pkg, d_info)


# ---- 1: the frame's winner, 12 floats at stride 48: the reference, the batch kernel, the device form ----------------------------------
@pytest.mark.parametrize("n,soa", [(65, False), (129, False), (129, True), (512, False), (6600, False)])
def test_the_winner_equals_the_reference_and_the_batch_form(pkg, O, reg, n, soa):
    sc = PF.scene(pkg, n)
    f = _frame(pkg, reg, sc.src, sc.tgt, soa)
    exp = PF.frame(O, sc.src, sc.tgt, [f["Rt"]], PF.TAU)
    got = reg.pose_info_frame(f["Rt"])
    _assert_info(got, exp, f"n={n} soa={soa} winner")
    assert int(got[0]["status"]) == SC_OK and int(got[0]["inliers"]) == f["stats"]["best_count"] >= 3  # the inlier test is the masks'
    assert reg.pose_info_frame(f["Rt"]).tobytes() == got.tobytes()                                     # the call may be repeated
    dev = _device(pkg, reg, pkg.make_pose_info_params(), f["Rt"].tobytes(), 48, 1)
    assert dev.tobytes() == got.tobytes()                                                              # host form == device form
    # the pose translated far away: an all-zero record with SC_OK, beside the winner's in one call
    two = reg.pose_info_frame(np.stack([PF.far(f["Rt"]), f["Rt"]]))
    assert two[0].tobytes() == bytes(REC) and two[1].tobytes() == got[0].tobytes()
    if n <= 512:  # GPU against GPU: sc_pose_info_batch on the same points and pose (it ends the frame, so it comes last)
        pose = np.zeros(1, pkg.BATCH_RESULT_DTYPE)
        pose["Rt"][0], pose["status"][0] = f["Rt"], SC_OK
        a, b = (np.ascontiguousarray(sc.src.T), np.ascontiguousarray(sc.tgt.T)) if soa else (sc.src, sc.tgt)
        bat = reg.pose_info_batch_raw(a, b, np.array([0, n], np.uint32), _params(pkg, soa), pose)
        assert bat.tobytes() == got.tobytes()


# ---- 2: the records of sc_polish_device as poses, stride 64, no flag (rank sits at byte 48) ---------------------------------------------
@pytest.mark.parametrize("n,cands", [(512, 8), (6600, 6)])
def test_polished_candidates_in_one_call(pkg, O, reg, n, cands):
    import torch
    sc = PF.scene(pkg, n)
    _frame(pkg, reg, sc.src, sc.tgt)
    q = pkg.make_polish_params(candidates=cands, max_iter=16)
    d_Rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_cand = torch.zeros(cands * 64, dtype=torch.uint8, device="cuda"); d_k = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_info = torch.full((cands * REC,), 0xAB, dtype=torch.uint8, device="cuda"); d_again = d_info.clone()
    torch.cuda.synchronize()
    rc, _ = reg.polish_device(q, d_Rt.data_ptr(), d_mask.data_ptr(), d_cand.data_ptr(), d_k.data_ptr())
    assert rc == SC_OK
    ip = pkg.make_pose_info_params()
    reg.pose_info_frame_device(ip, d_cand.data_ptr(), 64, cands, 0, d_info.data_ptr())
    reg.pose_info_frame_device(ip, d_cand.data_ptr(), 64, cands, 0, d_again.data_ptr())
    torch.cuda.synchronize()
    cand = np.frombuffer(d_cand.cpu().numpy().tobytes(), pkg.api.POLISH_CAND_DTYPE)
    K = int(d_k.cpu()[0])
    got = _records(pkg, d_info)
    print("candidates", K, "ranks", cand["rank"].tolist(), "scores", cand["score"].tolist())
    assert K >= 2 and (cand["rank"][:K] != 0).any()  # a non-zero word at byte 48 that is no status
    _assert_info(got, PF.frame(O, sc.src, sc.tgt, cand["Rt"], PF.TAU), f"n={n} candidates")
    assert np.array_equal(got["inliers"][:K], cand["score"][:K])  # inlier-count mode: the polished score is the count
    assert _records(pkg, d_again).tobytes() == got.tobytes()        # a repeated call is byte-identical
    # the same poses permuted give the records permuted; a record does not depend on n_poses
    order = np.roll(np.arange(cands), 3)[::-1].copy()
    perm = _device(pkg, reg, ip, cand[order].tobytes(), 64, cands)
    assert perm.tobytes() == got[order].tobytes()
    assert _device(pkg, reg, ip, cand[1:2].tobytes(), 64, 1).tobytes() == got[1:2].tobytes()


# ---- 3: SC_POSE_INFO_STATUS: a status is passed through, a NaN is its own pose's --------------------------------------------------------
def test_statuses_affect_only_their_own_pose(pkg, O, reg):
    sc = PF.scene(pkg, 129)
    f = _frame(pkg, reg, sc.src, sc.tgt)
    other = PF.rt_of(sc.R_gt, sc.t_gt)
    for dt in (pkg.BATCH_RESULT_DTYPE, pkg.api.POLISH_BATCH_RESULT_DTYPE):  # stride 80 and stride 64
        pose = np.zeros(5, dt)
        pose["Rt"] = [f["Rt"], other, f["Rt"], other, f["Rt"]]
        pose["status"] = [SC_OK, SC_ENOHYP, SC_OK, SC_OK, SC_OK]
        pose["Rt"][2][7] = np.nan
        exp = PF.frame(O, sc.src, sc.tgt, pose["Rt"], PF.TAU, statuses=pose["status"])
        got = reg.pose_info_frame(pose, flags=pkg.SC_POSE_INFO_STATUS)
        _assert_info(got, exp, f"stride {dt.itemsize} with the flag")
        assert list(got["status"]) == [SC_OK, SC_ENOHYP, SC_EINVAL, SC_OK, SC_OK]
        assert got[1].tobytes() == _zero(SC_ENOHYP) and got[2].tobytes() == _zero(SC_EINVAL)
        assert int(got[0]["inliers"]) >= 3 and int(got[3]["inliers"]) >= 3 and got[4].tobytes() == got[0].tobytes()
        assert _device(pkg, reg, pkg.make_pose_info_params(flags=pkg.SC_POSE_INFO_STATUS), pose.tobytes(), dt.itemsize, 5).tobytes() == got.tobytes()
        # without the flag the word at byte 48 is not read: pose 1 gets its matrix
        plain = reg.pose_info_frame(pose)
        _assert_info(plain, PF.frame(O, sc.src, sc.tgt, pose["Rt"], PF.TAU), f"stride {dt.itemsize} without the flag")
        assert int(plain[1]["status"]) == SC_OK and plain[1].tobytes() == got[3].tobytes()


# ---- 4: SEL_MASK after a peel round; the frame is untouched ----------------------------------------------------------------------------
def _flat(res):
    return dict(status=res["status"], Rt=np.concatenate([res["R"].ravel(), res["t"]]).astype(np.float32), mask=res["mask"],
                stats={k: res["stats"][k] for k in STAT_KEYS})


def _same(a, b, what):
    assert a["status"] == b["status"] and np.array_equal(a["mask"], b["mask"]) and a["Rt"].tobytes() == b["Rt"].tobytes(), what
    assert a["stats"] == b["stats"], what


def test_mask_of_a_peel_round_and_the_frame_stays_untouched(pkg, O):
    sc = PF.motions(pkg)
    with_info, without = pkg.Registrar(0), pkg.Registrar(0)
    try:
        f = _frame(pkg, with_info, sc.src, sc.tgt)
        _frame(pkg, without, sc.src, sc.tgt)
        r1 = _flat(with_info.peel())
        _same(r1, _flat(without.peel()), "round 1")
        assert r1["status"] == SC_OK
        # peel a round, take its information matrix (and the frame's winner's with its own mask) ...
        got = with_info.pose_info_frame(r1["Rt"], sel_mode=pkg.SC_POSE_INFO_SEL_MASK, sel=r1["mask"])
        _assert_info(got, PF.frame(O, sc.src, sc.tgt, [r1["Rt"]], PF.TAU, PF.SEL_MASK, r1["mask"]), "round 1 with its mask")
        assert int(got[0]["inliers"]) == r1["stats"]["best_count"] == int(r1["mask"].sum()) >= 3  # inlier-count mode
        dev = _device(pkg, with_info, pkg.make_pose_info_params(sel_mode=pkg.SC_POSE_INFO_SEL_MASK), r1["Rt"].tobytes(), 48, 1, r1["mask"])
        assert dev.tobytes() == got.tobytes()
        got0 = with_info.pose_info_frame(f["Rt"], sel_mode=pkg.SC_POSE_INFO_SEL_MASK, sel=f["mask"])
        _assert_info(got0, PF.frame(O, sc.src, sc.tgt, [f["Rt"]], PF.TAU, PF.SEL_MASK, f["mask"]), "the frame's winner with its mask")
        assert int(got0[0]["inliers"]) == f["stats"]["best_count"]
        # the mask is the same set for every pose: round 1's pose on the winner's correspondences holds next to nothing
        both = with_info.pose_info_frame(np.stack([f["Rt"], r1["Rt"]]), sel_mode=pkg.SC_POSE_INFO_SEL_MASK, sel=f["mask"])
        _assert_info(both, PF.frame(O, sc.src, sc.tgt, [f["Rt"], r1["Rt"]], PF.TAU, PF.SEL_MASK, f["mask"]), "two poses, one mask")
        assert both[0].tobytes() == got0[0].tobytes() and int(both[1]["inliers"]) < int(got[0]["inliers"])
        # ... peel the next: Rt, mask and stats are those of the context that made no info call; sc_polish likewise
        _same(_flat(with_info.peel()), _flat(without.peel()), "round 2")
        pa, pb = with_info.polish(candidates=4, max_iter=8), without.polish(candidates=4, max_iter=8)
        _same(_flat(pa), _flat(pb), "polish")
        assert pa["n_cand"] == pb["n_cand"] and pa["cand"].tobytes() == pb["cand"].tobytes()
        assert with_info.pose_info_frame(r1["Rt"], sel_mode=pkg.SC_POSE_INFO_SEL_MASK, sel=r1["mask"]).tobytes() == got.tobytes()
    finally:
        with_info.close(); without.close()


# ---- 5: SEL_LABEL with the outputs of sc_register_instances ---------------------------------------------------------------------------
def test_labels_of_register_instances(pkg, O, reg):
    sc = PF.motions(pkg)
    inst = reg.register_instances(sc.src, sc.tgt, max_instances=4, min_score=20, params=_params(pkg))
    Rt, score, label = inst["Rt"], inst["score"], inst["label"]
    print("motions", len(Rt), "scores", score.tolist())
    assert inst["status"] == SC_OK and len(Rt) >= 2 and (score >= 20).all()
    got = reg.pose_info_frame(Rt, sel_mode=pkg.SC_POSE_INFO_SEL_LABEL, sel=label)
    _assert_info(got, PF.frame(O, sc.src, sc.tgt, Rt, PF.TAU, PF.SEL_LABEL, label), "all motions in one call")
    assert np.array_equal(got["inliers"], score)  # inlier-count mode: what each motion claimed
    # label0 shifted, with the labels shifted alike, gives the same records
    shifted = reg.pose_info_frame(Rt, sel_mode=pkg.SC_POSE_INFO_SEL_LABEL, sel=label + 7, label0=7)
    assert shifted.tobytes() == got.tobytes()
    neg = reg.pose_info_frame(Rt, sel_mode=pkg.SC_POSE_INFO_SEL_LABEL, sel=label - 5, label0=-5)
    assert neg.tobytes() == got.tobytes()
    # one motion alone, found through label0: a record does not depend on k or on n_poses
    alone = reg.pose_info_frame(Rt[1], sel_mode=pkg.SC_POSE_INFO_SEL_LABEL, sel=label, label0=1)
    assert alone[0].tobytes() == got[1].tobytes()
    dev = _device(pkg, reg, pkg.make_pose_info_params(sel_mode=pkg.SC_POSE_INFO_SEL_LABEL), np.ascontiguousarray(Rt).tobytes(), 48, len(Rt), label)
    assert dev.tobytes() == got.tobytes()
    assert reg.peel()["status"] in (SC_OK, SC_ENOHYP)  # rounds may still follow: the frame is there


# ---- 6: crafted selections -----------------------------------------------------------------------------------------------------------
def test_crafted_selections(pkg, O, reg):
    src, tgt, Rt, sel = PF.crafted_hole()  # a mask that clears a whole middle chunk
    _frame(pkg, reg, src, tgt)
    full = reg.pose_info_frame(Rt)
    holed = reg.pose_info_frame(Rt, sel_mode=pkg.SC_POSE_INFO_SEL_MASK, sel=sel)
    _assert_info(full, PF.frame(O, src, tgt, [Rt], PF.TAU), "hole: no selection")
    _assert_info(holed, PF.frame(O, src, tgt, [Rt], PF.TAU, PF.SEL_MASK, sel), "hole: the middle chunk cleared")
    assert int(full[0]["inliers"]) == 96 and int(holed[0]["inliers"]) == 64
    assert reg.pose_info_frame(PF.far(Rt), sel_mode=pkg.SC_POSE_INFO_SEL_MASK, sel=sel)[0].tobytes() == bytes(REC)
    assert reg.pose_info_frame(Rt, sel_mode=pkg.SC_POSE_INFO_SEL_MASK, sel=np.zeros(192, np.uint8))[0].tobytes() == bytes(REC)
    src, tgt, Rt, sel = PF.crafted_last()  # a mask that leaves one inlier alone, in the last, partial chunk
    _frame(pkg, reg, src, tgt)
    last = reg.pose_info_frame(Rt, sel_mode=pkg.SC_POSE_INFO_SEL_MASK, sel=sel)
    _assert_info(last, PF.frame(O, src, tgt, [Rt], PF.TAU, PF.SEL_MASK, sel), "last: index 128 alone")
    assert int(last[0]["inliers"]) == 1 and int(last[0]["status"]) == SC_OK


# ---- 7: what is refused, and what a refused call leaves --------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_frame(pkg, O):
    import torch
    L = pkg.load_library()
    sc = PF.scene(pkg, 129)
    r = pkg.Registrar(0)
    try:
        pose = np.zeros(2, pkg.BATCH_RESULT_DTYPE)
        info = np.zeros(2, PF.RESULT_DTYPE)
        sel = np.ones(129, np.uint8)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

        def call(ip, stride=80, k=2, sel=None, pose=pose, info=info, entry=L.sc_pose_info_frame):
            rc = entry(r._h, None if ip is None else C.byref(ip), vp(pose), stride, k, vp(sel), vp(info))
            return rc, L.sc_last_error(r._h).decode()

        ok = pkg.make_pose_info_params()
        rc, text = call(ok)  # no frame on a fresh context
        assert rc == SC_EINVAL and "no frame" in text and "sc_pose_info_frame" in text
        f = _frame(pkg, r, sc.src, sc.tgt)
        pose["Rt"], pose["status"] = f["Rt"], SC_OK
        good = r.pose_info_frame(pose)
        assert good.tobytes() == PF.frame(O, sc.src, sc.tgt, pose["Rt"], PF.TAU).tobytes()
        short = pkg.make_pose_info_params(); short.size = 28
        res = pkg.make_pose_info_params(); res.reserved[3] = 1
        cases = {
            "ip NULL": (lambda: call(None), "NULL"),
            "pose NULL": (lambda: call(ok, pose=None), "NULL"),
            "info NULL": (lambda: call(ok, info=None), "NULL"),
            "size": (lambda: call(short), "size"),
            "sel_mode 3": (lambda: call(pkg.make_pose_info_params(sel_mode=3), sel=sel), "sel_mode"),
            "mask without sel": (lambda: call(pkg.make_pose_info_params(sel_mode=1)), "sel is NULL"),
            "label without sel": (lambda: call(pkg.make_pose_info_params(sel_mode=2)), "sel is NULL"),
            "label0 with no selection": (lambda: call(pkg.make_pose_info_params(label0=1)), "label0"),
            "label0 with a mask": (lambda: call(pkg.make_pose_info_params(sel_mode=1, label0=-1), sel=sel), "label0"),
            "flag 2": (lambda: call(pkg.make_pose_info_params(flags=2)), "flag"),
            "flag 3": (lambda: call(pkg.make_pose_info_params(flags=3)), "flag"),
            "reserved": (lambda: call(res), "reserved"),
            "n_poses 0": (lambda: call(ok, k=0), "n_poses"),
            "n_poses 1025": (lambda: call(ok, k=1025), "n_poses"),
            "stride 0": (lambda: call(ok, stride=0), "pose_stride"),
            "stride 44": (lambda: call(ok, stride=44), "pose_stride"),
            "stride 50": (lambda: call(ok, stride=50), "pose_stride"),
            "stride 48 with the flag": (lambda: call(pkg.make_pose_info_params(flags=1), stride=48), "pose_stride"),
            "device form, stride 50": (lambda: call(ok, stride=50, entry=L.sc_pose_info_frame_device), "sc_pose_info_frame_device"),
        }
        for what, (fn, word) in cases.items():
            rc, text = fn()
            print(what, rc, text)
            assert rc == SC_EINVAL and word in text and "sc_pose_info_frame" in text, what
            assert r.pose_info_frame(pose).tobytes() == good.tobytes(), what  # the refused call left the context and the frame
        assert L.sc_pose_info_frame(None, C.byref(ok), vp(pose), 80, 2, None, vp(info)) == SC_EINVAL
        # a batch entry ends the frame
        s2, t2 = batch_ref.scene(pkg, 128, .3)
        r.register_batch_raw(s2, t2, np.array([0, 128], np.uint32), _params(pkg))
        rc, text = call(ok)
        assert rc == SC_EINVAL and "no frame" in text
        # a frame call that returned SC_ENOHYP leaves no frame (three collinear, equidistant correspondences: no rotation)
        line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
        assert r.register(line, line, params=pkg.make_params(sigma=0.1, t_cmp=0.9, tau=0.1, min_len=0.1, max_triangles=10))["status"] == SC_ENOHYP
        rc, text = call(ok)
        assert rc == SC_EINVAL and "no frame" in text
        # a call outstanding
        ds, dt = torch.from_numpy(sc.src).cuda(), torch.from_numpy(sc.tgt).cuda()
        d_Rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_mask = torch.zeros(129, dtype=torch.uint8, device="cuda")
        r.register_device_async(ds.data_ptr(), dt.data_ptr(), 129, _params(pkg), d_Rt.data_ptr(), d_mask.data_ptr())
        rc, text = call(ok)
        assert rc == SC_EINVAL and "outstanding" in text
        assert r.wait()[0] == SC_OK
        assert r.pose_info_frame(pose).tobytes() == good.tobytes()  # a record does not depend on how the frame was enqueued
    finally:
        r.close()


# ---- 8: the workspace: allocated by the first call, held against the frame's cap --------------------------------------------------------
def test_workspace_appears_with_the_first_call_and_respects_the_cap(pkg, O):
    sc = PF.scene(pkg, 6600)
    nch = (6600 + 63) // 64
    r = pkg.Registrar(0)
    try:
        r.set_debug(no_fast=1)  # (the same input takes the same path every time: what moves afterwards is these entries')
        p = _params(pkg)
        held = [r.register(sc.src, sc.tgt, params=p)["stats"]["workspace_bytes"] for _ in range(4)]
        assert held[2] == held[3] > 0, held
        f = _frame(pkg, r, sc.src, sc.tgt)
        poses = np.tile(f["Rt"], (64, 1))
        got = r.pose_info_frame(poses)
        assert r.peel()["status"] in (SC_OK, SC_ENOHYP)  # (the rounds' own workspace exists from here on)
        after = r.register(sc.src, sc.tgt, params=p)["stats"]["workspace_bytes"]
        print(held, after)
        assert after >= held[3] + 64 * nch * 128 + 64 * 48 + 64 * REC  # the chunk sums' scratch and the host form's copies
        assert r.pose_info_frame(poses).tobytes() == got.tobytes()
        assert r.register(sc.src, sc.tgt, params=p)["stats"]["workspace_bytes"] == after
        assert len({g.tobytes() for g in got}) == 1 and int(got[0]["inliers"]) == f["stats"]["best_count"]
        # a cap with no room for the scratch: SC_ENOMEM, nothing enqueued, the context and the frame stay usable
        fc = _frame(pkg, r, sc.src, sc.tgt, max_workspace=after + 4096)
        assert fc["Rt"].tobytes() == f["Rt"].tobytes()
        with pytest.raises(pkg.SacCotError) as e:
            r.pose_info_frame(np.tile(f["Rt"], (1024, 1)))  # 1024 x 104 x 128 bytes of chunk sums
        assert e.value.status == SC_ENOMEM
        assert r.pose_info_frame(poses).tobytes() == got.tobytes()  # ... what fits still runs, on the same frame
        assert r.peel()["status"] in (SC_OK, SC_ENOHYP)                # ... and so does a round
    finally:
        r.close()
