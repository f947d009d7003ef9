"""GPU: caller-supplied poses refitted to a fixed point on a scored frame (include/saccot.h, sc_polish_poses / sc_polish_poses_device).

The expected value of every case is tests/polish_poses_ref.py — polish_ref.iterate's loop on the CPU restatement's O.mask / O.refine /
O.score with the selection ANDed into every inlier set — and every comparison is bit for bit: the 64 bytes of every record (`tobytes`)
and every mask byte.  No tolerances.  The equalities the header promises are checked GPU against GPU as well: sc_polish, sc_polish_cand
records, sc_polish_batch, SC_FLAG_REFINE of sc_register_instances and of sc_peel.  The scenes are checked on the CPU by
tests/test_polish_poses_abi.py.
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref
import polish_poses_ref as PF
import polish_ref

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOMEM, SC_ENOHYP = 0, -1, -2, -5
SC_FLAG_REFINE = 8
REC = 64
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


def _assert_pol(got, exp, what=""):
    (g_rec, g_mask), (e_rec, e_mask) = got, exp
    assert len(g_rec) == len(e_rec), what
    for k in range(len(g_rec)):
        g, e = g_rec[k], e_rec[k]
        print(what, k, *[int(g[f]) for f in ("status", "score0", "score", "iters", "stop")], "| expected",
              *[int(e[f]) for f in ("status", "score0", "score", "iters", "stop")])
        assert g.tobytes() == e.tobytes(), (what, k)
        if g_mask is not None:
            assert np.array_equal(g_mask[k], e_mask[k]), (what, k)


def _none(status):
    z = np.zeros((), PF.RESULT_DTYPE); z["Rt"], z["stop"], z["status"] = PF.IDENT, PF.STOP_DECLINED, status
    return z.tobytes()


def _device(pkg, r, qp, pose_bytes, stride, k, n, sel=None, want_mask=True):
    """the device form on host data: copies in, one call, one device-wide wait -> (records (k,), masks (k, n) or None)"""
    import torch
    d_pose = torch.from_numpy(np.frombuffer(pose_bytes, np.uint8).copy()).cuda()
    d_sel = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel)).cuda()
    d_pol = torch.full((k * REC,), 0xAB, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((k * n,), 0xAB, dtype=torch.uint8, device="cuda") if want_mask else None
    torch.cuda.synchronize()
    r.polish_poses_device(qp, d_pose.data_ptr(), stride, k, 0 if d_sel is None else d_sel.data_ptr(), d_pol.data_ptr(),
                          0 if d_mask is None else d_mask.data_ptr())
    torch.cuda.synchronize()
    assert d_pose.cpu().numpy().tobytes() == pose_bytes  # d_pose is read, never written
    rec = np.frombuffer(d_pol.cpu().numpy().tobytes(), pkg.POLISH_BATCH_RESULT_DTYPE)
    return rec, (None if d_mask is None else d_mask.cpu().numpy().reshape(k, n))


# ---- 1: the frame's winner: the reference, sc_polish(candidates = 1), sc_polish_batch (promises 1 and 3), the device form -------------
@pytest.mark.parametrize("n,soa", [(65, False), (129, False), (129, True), (512, False), (7400, False)])
def test_the_winner_equals_the_reference_polish_and_the_batch_form(pkg, O, reg, n, soa):
    sc = PF.scene(pkg, n)
    f = _frame(pkg, reg, sc.src, sc.tgt, soa)
    for max_iter in (1, 16):
        exp = PF.poses(O, sc.src, sc.tgt, [f["Rt"]], PF.TAU, max_iter=max_iter)
        got = reg.polish_poses(f["Rt"], max_iter=max_iter)
        _assert_pol(got, exp, f"n={n} soa={soa} max_iter={max_iter} winner")
        rec, mask = got
        assert int(rec[0]["status"]) == SC_OK and int(rec[0]["score0"]) == f["stats"]["best_count"] >= 3
        again = reg.polish_poses(f["Rt"], max_iter=max_iter)                                 # the call may be repeated
        assert again[0].tobytes() == rec.tobytes() and np.array_equal(again[1], mask)
        qp = pkg.make_polish_poses_params(max_iter=max_iter)
        dev = _device(pkg, reg, qp, f["Rt"].tobytes(), 48, 1, n)                             # host form == device form
        assert dev[0].tobytes() == rec.tobytes() and np.array_equal(dev[1], mask)
        assert _device(pkg, reg, qp, f["Rt"].tobytes(), 48, 1, n, want_mask=False)[0].tobytes() == rec.tobytes()  # d_mask NULL
        # promise 1: sc_polish(candidates = 1, the same max_iter) on the same frame
        pol = reg.polish(candidates=1, max_iter=max_iter)
        c = pol["cand"][0]
        assert pol["status"] == SC_OK and pol["n_cand"] == 1
        assert c["Rt"].tobytes() == rec[0]["Rt"].tobytes() and np.array_equal(pol["mask"], mask[0])
        assert (int(c["score0"]), int(c["score"]), int(c["iters"])) == (int(rec[0]["score0"]), int(rec[0]["score"]), int(rec[0]["iters"]))
    assert int(rec[0]["iters"]) >= 1  # (max_iter = 16: a refit that changed (R, t) went through the chains)
    # the pose translated far away is declined, beside the winner's in one call
    two = reg.polish_poses(np.stack([PF.far(f["Rt"]), f["Rt"]]))
    _assert_pol(two, PF.poses(O, sc.src, sc.tgt, [PF.far(f["Rt"]), f["Rt"]], PF.TAU), "far + winner")
    assert two[0][1].tobytes() == rec[0].tobytes() and two[0][0]["Rt"].tobytes() == PF.far(f["Rt"]).tobytes()
    assert [int(two[0][0][x]) for x in ("status", "score0", "score", "iters", "stop")] == [SC_OK, 0, 0, 0, PF.STOP_DECLINED]
    if n <= 512:  # promise 3, GPU against GPU: sc_polish_batch on the same points and pose (it ends the frame, so it comes last)
        pose = np.zeros(1, pkg.BATCH_RESULT_DTYPE)
        pose["Rt"][0], pose["status"][0] = f["Rt"], SC_OK
        a, b = (np.ascontiguousarray(sc.src.T), np.ascontiguousarray(sc.tgt.T)) if soa else (sc.src, sc.tgt)
        bat, bmask = reg.polish_batch_raw(a, b, np.array([0, n], np.uint32), _params(pkg, soa), pkg.make_polish_params(candidates=1, max_iter=16), pose)
        assert bat.tobytes() == rec.tobytes() and np.array_equal(bmask, mask[0])


# ---- 2: hypotheses of the ranked list against sc_polish's records (promise 2); permutations; n_poses ------------------------------------
@pytest.mark.parametrize("n,cands", [(512, 8), (7400, 6)])
def test_hypotheses_equal_their_polish_cand_records(pkg, O, reg, n, cands):
    sc = PF.scene(pkg, n)
    _frame(pkg, reg, sc.src, sc.tgt)
    hyp = polish_ref.hypotheses(O, sc.src, sc.tgt, PF.kw_of(), threads=min(O.max_threads(), 16))
    pol = reg.polish(candidates=cands, max_iter=16)
    K, cand = pol["n_cand"], pol["cand"]
    print("candidates", K, "ranks", cand["rank"].tolist(), "scores", cand["score"].tolist())
    assert pol["status"] == SC_OK and K == cands and (cand["rank"][:K] != 0).any()
    poses = np.ascontiguousarray(hyp["Rt"][cand["rank"][:K]])  # the CPU restatement's hypotheses at the candidates' ranks
    exp = PF.poses(O, sc.src, sc.tgt, poses, PF.TAU)
    got = reg.polish_poses(poses)
    _assert_pol(got, exp, f"n={n} hypotheses")
    rec, mask = got
    for k in range(K):
        assert rec[k]["Rt"].tobytes() == cand[k]["Rt"].tobytes(), k
        assert [int(rec[k][x]) for x in ("score0", "score", "iters")] == [int(cand[k][x]) for x in ("score0", "score", "iters")], k
    # sc_polish's own records as poses: stride 64, no flag — the rank at byte 48 is not a status; the fixed points return themselves
    fed = reg.polish_poses(cand[:K])
    _assert_pol(fed, PF.poses(O, sc.src, sc.tgt, cand["Rt"][:K], PF.TAU), "cand records fed in")
    # the same poses permuted give the records and masks permuted; a record does not depend on n_poses
    order = np.roll(np.arange(K), 3)[::-1].copy()
    qp = pkg.make_polish_poses_params()
    perm = _device(pkg, reg, qp, poses[order].tobytes(), 48, K, n)
    assert perm[0].tobytes() == rec[order].tobytes() and np.array_equal(perm[1], mask[order])
    alone = _device(pkg, reg, qp, poses[1:2].tobytes(), 48, 1, n)
    assert alone[0].tobytes() == rec[1:2].tobytes() and np.array_equal(alone[1], mask[1:2])


# ---- 3: the four selections on the crafted labels ------------------------------------------------------------------------------------
def test_the_four_selections_on_the_crafted_labels(pkg, O, reg):
    sc, label = PF.motions(pkg)
    n = len(sc.src)
    _frame(pkg, reg, sc.src, sc.tgt)
    poses = np.stack([PF.rt_of(R, t) for R, t in sc.motions])
    got = {}
    for name, mode in (("none", PF.SEL_NONE), ("label", PF.SEL_LABEL), ("alive", PF.SEL_ALIVE)):
        sel = None if mode == PF.SEL_NONE else label
        got[name] = reg.polish_poses(poses, sel_mode=mode, sel=sel)
        _assert_pol(got[name], PF.poses(O, sc.src, sc.tgt, poses, PF.TAU, mode, sel), name)
        if sel is not None:  # label0 = 7 with the labels shifted alike gives the same bytes; so does a negative label0
            for shift in (7, -5):
                sh = reg.polish_poses(poses, sel_mode=mode, sel=label + shift, label0=shift)
                assert sh[0].tobytes() == got[name][0].tobytes() and np.array_equal(sh[1], got[name][1]), (name, shift)
            dev = _device(pkg, reg, pkg.make_polish_poses_params(sel_mode=mode), poses.tobytes(), 48, 2, n, label)
            assert dev[0].tobytes() == got[name][0].tobytes() and np.array_equal(dev[1], got[name][1])
    for a, b in (("none", "alive"), ("none", "label"), ("alive", "label")):  # a kernel that ignored or confused the modes could not pass
        assert got[a][0][1].tobytes() != got[b][0][1].tobytes()
    assert (label[np.flatnonzero(got["alive"][1][1])] == -1).any() and not (label[np.flatnonzero(got["alive"][1][1])] == 0).any()
    assert (label[np.flatnonzero(got["label"][1][1])] == 1).all()
    # SEL_MASK: one set for every pose — pose 1's ALIVE set gives pose 1's ALIVE record at k = 0 and at k = 1
    alive1 = PF.part_of(n, 1, PF.SEL_ALIVE, label).astype(np.uint8) * 9  # (any non-zero byte)
    m = reg.polish_poses(poses[[1, 0, 1]], sel_mode=PF.SEL_MASK, sel=alive1)
    _assert_pol(m, PF.poses(O, sc.src, sc.tgt, poses[[1, 0, 1]], PF.TAU, PF.SEL_MASK, alive1), "mask")
    assert m[0][0].tobytes() == m[0][2].tobytes() == got["alive"][0][1].tobytes() and np.array_equal(m[1][0], got["alive"][1][1])
    # one pose alone, found through label0: a record depends on k only through label0 + k
    for name, mode in (("label", PF.SEL_LABEL), ("alive", PF.SEL_ALIVE)):
        alone = reg.polish_poses(poses[1], sel_mode=mode, sel=label, label0=1)
        if mode == PF.SEL_LABEL:
            assert alone[0][0].tobytes() == got[name][0][1].tobytes() and np.array_equal(alone[1][0], got[name][1][1])
        else:  # ALIVE at k = 0 with label0 = 1: sel < 1 or sel >= 1 — everything
            assert alone[0][0].tobytes() == got["none"][0][1].tobytes()
    # a selection that leaves nothing: declined at once, a zero mask, the input's bits
    nothing = reg.polish_poses(poses, sel_mode=PF.SEL_MASK, sel=np.zeros(n, np.uint8))
    _assert_pol(nothing, PF.poses(O, sc.src, sc.tgt, poses, PF.TAU, PF.SEL_MASK, np.zeros(n, np.uint8)), "empty mask")
    assert not nothing[1].any() and nothing[0]["Rt"].tobytes() == poses.tobytes() and (nothing[0]["stop"] == PF.STOP_DECLINED).all()


# ---- 4: promises 4 and 5: SC_FLAG_REFINE of sc_register_instances and of sc_peel ---------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])  # SC_SCORE_COUNT and the truncated squared residual (a score is then up to 1024 per inlier)
def test_one_refit_equals_flag_refine_of_instances_and_peel(pkg, O, reg, mode):
    sc = pkg.synth.make_scene_motions(1500, [.25, .15], 1.0, PF.TAU, 7300)
    n = len(sc.src)
    min_score = 20 if mode == 0 else 20 * 1024
    plain = reg.register_instances(sc.src, sc.tgt, max_instances=4, min_score=min_score, params=_params(pkg, score_mode=mode))
    refined = reg.register_instances(sc.src, sc.tgt, max_instances=4, min_score=min_score,
                                     params=_params(pkg, score_mode=mode, flags=SC_FLAG_REFINE))
    K = len(plain["Rt"])
    print("motions", K, "scores", plain["score"].tolist())
    assert plain["status"] == refined["status"] == SC_OK and K == len(refined["Rt"]) >= 2
    assert np.array_equal(plain["label"], refined["label"]) and np.array_equal(plain["score"], refined["score"])
    assert plain["Rt"].tobytes() != refined["Rt"].tobytes()
    # the frame the second call left is the same frame (SC_FLAG_REFINE changes a frame's outputs, not what it stages)
    got = reg.polish_poses(plain["Rt"], sel_mode=PF.SEL_ALIVE, sel=plain["label"], max_iter=1)
    _assert_pol(got, PF.poses(O, sc.src, sc.tgt, plain["Rt"], PF.TAU, PF.SEL_ALIVE, plain["label"], score_mode=mode, max_iter=1), f"mode {mode} alive")
    rec, mask = got
    for k in range(K):
        assert rec[k]["Rt"].tobytes() == refined["Rt"][k].tobytes(), k
        assert int(rec[k]["score0"]) == int(refined["score"][k]), k
    # promise 5: a round of sc_peel on a frame with SC_FLAG_REFINE, against SEL_MASK with the round's mask and its fp32 pose
    _frame(pkg, reg, sc.src, sc.tgt, score_mode=mode, flags=SC_FLAG_REFINE)
    r_ref = reg.peel()
    f = _frame(pkg, reg, sc.src, sc.tgt, score_mode=mode)
    r_plain = reg.peel()
    assert r_ref["status"] == r_plain["status"] == SC_OK and np.array_equal(r_ref["mask"], r_plain["mask"])
    rt_plain = np.concatenate([r_plain["R"].ravel(), r_plain["t"]]).astype(np.float32)
    rt_ref = np.concatenate([r_ref["R"].ravel(), r_ref["t"]]).astype(np.float32)
    assert rt_plain.tobytes() == plain["Rt"][1].tobytes() and rt_ref.tobytes() != rt_plain.tobytes()
    one = reg.polish_poses(rt_plain, sel_mode=PF.SEL_MASK, sel=r_plain["mask"], max_iter=1)
    _assert_pol(one, PF.poses(O, sc.src, sc.tgt, [rt_plain], PF.TAU, PF.SEL_MASK, r_plain["mask"], score_mode=mode, max_iter=1), f"mode {mode} peel mask")
    assert one[0][0]["Rt"].tobytes() == rt_ref.tobytes() and int(one[0][0]["score0"]) == r_plain["stats"]["best_count"]
    # iterated to the fixed point, motion 1 with its alive set: the reference, and no worse a count than the single refit in count mode
    full = reg.polish_poses(plain["Rt"], sel_mode=PF.SEL_ALIVE, sel=plain["label"])
    _assert_pol(full, PF.poses(O, sc.src, sc.tgt, plain["Rt"], PF.TAU, PF.SEL_ALIVE, plain["label"], score_mode=mode), f"mode {mode} alive, 16")
    assert f["status"] == SC_OK


# ---- 5: SC_POLISH_POSES_STATUS; records fed back; the records as poses of sc_pose_info_frame ---------------------------------------------
def test_statuses_affect_only_their_own_pose(pkg, O, reg):
    sc = PF.scene(pkg, 129)
    f = _frame(pkg, reg, sc.src, sc.tgt)
    other = PF.rt_of(sc.R_gt, sc.t_gt)
    for dt in (pkg.BATCH_RESULT_DTYPE, pkg.api.POLISH_BATCH_RESULT_DTYPE):  # stride 80 and stride 64
        pose = np.zeros(5, dt)
        pose["Rt"] = [f["Rt"], other, f["Rt"], other, f["Rt"]]
        pose["status"] = [SC_OK, SC_ENOHYP, SC_OK, 77, SC_OK]
        pose["Rt"][2][7] = np.nan
        exp = PF.poses(O, sc.src, sc.tgt, pose["Rt"], PF.TAU, statuses=pose["status"])
        got = reg.polish_poses(pose, flags=pkg.SC_POLISH_POSES_STATUS)
        _assert_pol(got, exp, f"stride {dt.itemsize} with the flag")
        rec, mask = got
        assert list(rec["status"]) == [SC_OK, SC_ENOHYP, SC_EINVAL, 77, SC_OK]
        assert rec[1].tobytes() == _none(SC_ENOHYP) and rec[2].tobytes() == _none(SC_EINVAL) and rec[3].tobytes() == _none(77)
        assert not mask[1].any() and not mask[2].any() and not mask[3].any()
        assert int(rec[0]["score"]) >= 3 and rec[4].tobytes() == rec[0].tobytes() and np.array_equal(mask[4], mask[0])  # the neighbours are untouched
        dev = _device(pkg, reg, pkg.make_polish_poses_params(flags=pkg.SC_POLISH_POSES_STATUS), pose.tobytes(), dt.itemsize, 5, 129)
        assert dev[0].tobytes() == rec.tobytes() and np.array_equal(dev[1], mask)
        # without the flag the word at byte 48 is not read: poses 1 and 3 are polished
        plain = reg.polish_poses(pose)
        _assert_pol(plain, PF.poses(O, sc.src, sc.tgt, pose["Rt"], PF.TAU), f"stride {dt.itemsize} without the flag")
        assert int(plain[0][1]["status"]) == SC_OK and plain[0][1].tobytes() == plain[0][3].tobytes() and int(plain[0][1]["score"]) >= 3
    # ... and so is the rank of an sc_polish_cand record
    pol = reg.polish(candidates=4, max_iter=2)
    assert pol["n_cand"] == 4 and (pol["cand"]["rank"] != 0).any()
    _assert_pol(reg.polish_poses(pol["cand"]), PF.poses(O, sc.src, sc.tgt, pol["cand"]["Rt"], PF.TAU), "cand records, no flag")


def test_records_feed_back_and_feed_pose_info_frame(pkg, O, reg):
    import torch
    sc, label = PF.motions(pkg)
    n = len(sc.src)
    _frame(pkg, reg, sc.src, sc.tgt)
    poses = np.stack([PF.rt_of(R, t) for R, t in sc.motions] + [PF.far(PF.rt_of(*sc.motions[0]))])
    rec, mask = reg.polish_poses(poses)
    assert list(rec["stop"]) == [PF.STOP_FIXED, PF.STOP_FIXED, PF.STOP_DECLINED] and (rec["iters"][:2] >= 1).all()
    # a record fed back in as a pose (stride 64, the flag): the fixed point returns itself with iters 0
    back, bmask = reg.polish_poses(rec, flags=pkg.SC_POLISH_POSES_STATUS)
    _assert_pol((back, bmask), PF.poses(O, sc.src, sc.tgt, rec["Rt"], PF.TAU, statuses=rec["status"]), "fed back")
    for k in range(2):
        assert back[k]["Rt"].tobytes() == rec[k]["Rt"].tobytes() and np.array_equal(bmask[k], mask[k])
        assert [int(back[k][x]) for x in ("status", "score0", "score", "iters", "stop")] == [SC_OK, int(rec[k]["score"]), int(rec[k]["score"]), 0, PF.STOP_FIXED]
    # the device chain of INTEGRATION: sc_polish_poses_device -> sc_pose_info_frame_device on its records (stride 64, STATUS, SEL_NONE)
    d_pose = torch.from_numpy(poses).cuda()
    d_pol = torch.zeros(3 * REC, dtype=torch.uint8, device="cuda"); d_info = torch.zeros(3 * 320, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reg.polish_poses_device(pkg.make_polish_poses_params(), d_pose.data_ptr(), 48, 3, 0, d_pol.data_ptr(), 0)
    reg.pose_info_frame_device(pkg.make_pose_info_params(flags=pkg.SC_POSE_INFO_STATUS), d_pol.data_ptr(), 64, 3, 0, d_info.data_ptr())
    torch.cuda.synchronize()
    assert d_pol.cpu().numpy().tobytes() == rec.tobytes()
    info = np.frombuffer(d_info.cpu().numpy().tobytes(), pkg.POSE_INFO_RESULT_DTYPE)
    assert (info["status"] == SC_OK).all() and np.array_equal(info["inliers"], rec["score"]) and int(info["inliers"][2]) == 0  # count mode


# ---- 6: the frame is untouched -------------------------------------------------------------------------------------------------------
def _flat(res):
    return dict(status=res["status"], Rt=np.concatenate([res["R"].ravel(), res["t"]]).astype(np.float32), mask=res["mask"],
                stats={k: res["stats"][k] for k in STAT_KEYS})


def _same(a, b, what):
    assert a["status"] == b["status"] and np.array_equal(a["mask"], b["mask"]) and a["Rt"].tobytes() == b["Rt"].tobytes(), what
    assert a["stats"] == b["stats"], what


def test_the_frame_stays_untouched(pkg, O):
    sc, label = PF.motions(pkg)
    with_call, without = pkg.Registrar(0), pkg.Registrar(0)
    try:
        f = _frame(pkg, with_call, sc.src, sc.tgt)
        _frame(pkg, without, sc.src, sc.tgt)
        poses = np.stack([f["Rt"], PF.rt_of(*sc.motions[1])])
        got = with_call.polish_poses(poses, sel_mode=PF.SEL_ALIVE, sel=label)
        _assert_pol(got, PF.poses(O, sc.src, sc.tgt, poses, PF.TAU, PF.SEL_ALIVE, label), "before the round")
        r1 = _flat(with_call.peel())
        _same(r1, _flat(without.peel()), "round 1")
        assert r1["status"] == SC_OK
        # interleaved with the rounds, the polish and the information matrix: each equals that of the context that never made the call
        one = with_call.polish_poses(r1["Rt"], sel_mode=PF.SEL_MASK, sel=r1["mask"])
        _assert_pol(one, PF.poses(O, sc.src, sc.tgt, [r1["Rt"]], PF.TAU, PF.SEL_MASK, r1["mask"]), "round 1 with its mask")
        _same(_flat(with_call.peel()), _flat(without.peel()), "round 2")
        pa, pb = with_call.polish(candidates=4, max_iter=8), without.polish(candidates=4, max_iter=8)
        _same(_flat(pa), _flat(pb), "polish")
        assert pa["n_cand"] == pb["n_cand"] and pa["cand"].tobytes() == pb["cand"].tobytes()
        assert with_call.pose_info_frame(poses).tobytes() == without.pose_info_frame(poses).tobytes()
        again = with_call.polish_poses(poses, sel_mode=PF.SEL_ALIVE, sel=label)
        assert again[0].tobytes() == got[0].tobytes() and np.array_equal(again[1], got[1])
    finally:
        with_call.close(); without.close()


# ---- 7: what is refused, and what a refused call leaves --------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_frame(pkg, O):
    import torch
    L = pkg.load_library()
    sc = PF.scene(pkg, 129)
    r = pkg.Registrar(0)
    try:
        pose = np.zeros(2, pkg.BATCH_RESULT_DTYPE)
        pol = np.zeros(2, PF.RESULT_DTYPE)
        mask = np.zeros(2 * 129, np.uint8)
        sel = np.ones(129, np.uint8); lab = np.zeros(129, np.int32)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

        def call(qp, stride=80, k=2, sel=None, pose=pose, pol=pol, entry=L.sc_polish_poses):
            rc = entry(r._h, None if qp is None else C.byref(qp), vp(pose), stride, k, vp(sel), vp(pol), vp(mask))
            return rc, L.sc_last_error(r._h).decode()

        ok = pkg.make_polish_poses_params()
        rc, text = call(ok)  # no frame on a fresh context
        assert rc == SC_EINVAL and "no frame" in text and "sc_polish_poses" in text
        f = _frame(pkg, r, sc.src, sc.tgt)
        pose["Rt"], pose["status"] = f["Rt"], SC_OK
        good = r.polish_poses(pose)
        exp = PF.poses(O, sc.src, sc.tgt, pose["Rt"], PF.TAU)
        assert good[0].tobytes() == exp[0].tobytes() and np.array_equal(good[1], exp[1])
        short = pkg.make_polish_poses_params(); short.size = 28
        res = pkg.make_polish_poses_params(); res.reserved[2] = 1
        mk = pkg.make_polish_poses_params
        cases = {
            "qp NULL": (lambda: call(None), "NULL"),
            "pose NULL": (lambda: call(ok, pose=None), "NULL"),
            "pol NULL": (lambda: call(ok, pol=None), "NULL"),
            "size": (lambda: call(short), "size"),
            "max_iter 0": (lambda: call(mk(max_iter=0)), "max_iter"),
            "max_iter 65": (lambda: call(mk(max_iter=65)), "max_iter"),
            "sel_mode 4": (lambda: call(mk(sel_mode=4), sel=sel), "sel_mode"),
            "mask without sel": (lambda: call(mk(sel_mode=1)), "sel is NULL"),
            "label without sel": (lambda: call(mk(sel_mode=2)), "sel is NULL"),
            "alive without sel": (lambda: call(mk(sel_mode=3)), "sel is NULL"),
            "label0 with no selection": (lambda: call(mk(label0=1)), "label0"),
            "label0 with a mask": (lambda: call(mk(sel_mode=1, label0=-1), sel=sel), "label0"),
            "flag 2": (lambda: call(mk(flags=2)), "flag"),
            "flag 3": (lambda: call(mk(flags=3)), "flag"),
            "reserved": (lambda: call(res), "reserved"),
            "n_poses 0": (lambda: call(ok, k=0), "n_poses"),
            "n_poses 1025": (lambda: call(ok, k=1025), "n_poses"),
            "stride 0": (lambda: call(ok, stride=0), "pose_stride"),
            "stride 44": (lambda: call(ok, stride=44), "pose_stride"),
            "stride 50": (lambda: call(ok, stride=50), "pose_stride"),
            "stride 48 with the flag": (lambda: call(mk(flags=1), stride=48), "pose_stride"),
            "device form, stride 50": (lambda: call(ok, stride=50, entry=L.sc_polish_poses_device), "sc_polish_poses_device"),
        }
        for what, (fn, word) in cases.items():
            rc, text = fn()
            print(what, rc, text)
            assert rc == SC_EINVAL and word in text and "sc_polish_poses" in text, what
            again = r.polish_poses(pose)
            assert again[0].tobytes() == good[0].tobytes() and np.array_equal(again[1], good[1]), what  # the refused call left the context and the frame
        assert L.sc_polish_poses(None, C.byref(ok), vp(pose), 80, 2, None, vp(pol), None) == SC_EINVAL
        # label0 is allowed with both label modes
        for mode in (2, 3):
            assert call(mk(sel_mode=mode, label0=5), sel=lab)[0] == SC_OK
        # a batch entry ends the frame
        s2, t2 = batch_ref.scene(pkg, 128, .3)
        r.register_batch_raw(s2, t2, np.array([0, 128], np.uint32), _params(pkg))
        rc, text = call(ok)
        assert rc == SC_EINVAL and "no frame" in text
        # a call outstanding
        ds, dt = torch.from_numpy(sc.src).cuda(), torch.from_numpy(sc.tgt).cuda()
        d_Rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_mask = torch.zeros(129, dtype=torch.uint8, device="cuda")
        r.register_device_async(ds.data_ptr(), dt.data_ptr(), 129, _params(pkg), d_Rt.data_ptr(), d_mask.data_ptr())
        rc, text = call(ok)
        assert rc == SC_EINVAL and "outstanding" in text
        assert r.wait()[0] == SC_OK
        again = r.polish_poses(pose)  # a record does not depend on how the frame was enqueued
        assert again[0].tobytes() == good[0].tobytes() and np.array_equal(again[1], good[1])
    finally:
        r.close()


# ---- 8: the workspace: allocated by the first call, held against the frame's cap --------------------------------------------------------
def test_workspace_appears_with_the_first_call_and_respects_the_cap(pkg, O):
    n = 7400
    sc = PF.scene(pkg, n)
    nch = (n + 63) // 64
    r = pkg.Registrar(0)
    try:
        r.set_debug(no_fast=1)  # (the same input takes the same path every time: what moves afterwards is these entries')
        p = _params(pkg)
        held = [r.register(sc.src, sc.tgt, params=p)["stats"]["workspace_bytes"] for _ in range(4)]
        assert held[2] == held[3] > 0, held
        f = _frame(pkg, r, sc.src, sc.tgt)
        poses = np.tile(f["Rt"], (64, 1))
        got = r.polish_poses(poses)
        assert r.peel()["status"] in (SC_OK, SC_ENOHYP)  # (the rounds' own workspace exists from here on)
        after = r.register(sc.src, sc.tgt, params=p)["stats"]["workspace_bytes"]
        print(held, after)
        assert after >= held[3] + 64 * nch * 128 + 64 * 48 + 64 * REC + 64 * n  # the chunk sums' scratch and the host form's copies
        again = r.polish_poses(poses)
        assert again[0].tobytes() == got[0].tobytes() and np.array_equal(again[1], got[1])
        assert r.register(sc.src, sc.tgt, params=p)["stats"]["workspace_bytes"] == after
        assert len({g.tobytes() for g in got[0]}) == 1 and int(got[0][0]["score0"]) == f["stats"]["best_count"]
        assert (got[1] == got[1][0]).all()
        # a cap with no room for the scratch: SC_ENOMEM, nothing enqueued, the context and the frame stay usable
        fc = _frame(pkg, r, sc.src, sc.tgt, max_workspace=after + 4096)
        assert fc["Rt"].tobytes() == f["Rt"].tobytes()
        with pytest.raises(pkg.SacCotError) as e:
            r.polish_poses(np.tile(f["Rt"], (1024, 1)))  # 1024 x 116 x 128 bytes of chunk sums, 1024 x n mask bytes
        assert e.value.status == SC_ENOMEM
        with pytest.raises(pkg.SacCotError) as e:
            r.polish_poses(np.tile(f["Rt"], (1024, 1)), want_mask=False)  # the scratch alone does not fit either
        assert e.value.status == SC_ENOMEM
        again = r.polish_poses(poses)  # ... what fits still runs, on the same frame
        assert again[0].tobytes() == got[0].tobytes() and np.array_equal(again[1], got[1])
        assert r.peel()["status"] in (SC_OK, SC_ENOHYP)  # ... and so does a round
    finally:
        r.close()
