"""GPU: correspondences of a scored frame labelled by the pose that fits best (include/saccot.h, sc_assign_poses_frame /
sc_assign_poses_frame_device).

The expected value of every case is tests/assign_ref.py — an exact emulation of the canonical fp32 residual, pinned to the CPU
restatement by tests/test_assign_abi.py — and every comparison is bit for bit: every label, every residual's bits, the 32 bytes of
every record.  No tolerances.  The equalities the header promises are checked GPU against GPU as well: sc_mask_host, the label and
scores of sc_register_instances (in every score mode: tests/test_assign_abi.py confirmed the two truncated ones on the reference),
sc_pose_info_frame under SEL_LABEL, and the device-side loop of INTEGRATION.md against the same loop on the references.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import assign_ref as AR
import batch_ref
import polish_poses_ref as PF
import pose_info_frame_ref as PIF
from test_assign_abi import CONFIRMED_SCORE_MODES
from test_range_oracle import WIN_C2, WIN_REGISTER, in_window, pow2, scaled, scaled_kw

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOMEM, SC_ENOHYP = 0, -1, -2, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = int(re.search(r"constexpr int ASSIGN_TILE = (\d+);", open(os.path.join(ROOT, "sac-cot_amd", "csrc", "sc_assign.hpp")).read()).group(1))
REC = 32
STAT_KEYS = ("n", "edges", "tri_total", "tri_kept", "tri_scored", "best_rank", "best_count")


def test_the_tile_is_what_the_sizes_assume():
    assert 129 < T <= 4096 and 7400 > T + 1  # T - 1 and T + 1 sit either side of one tile; 7400 spans several


def _params(pkg, soa=False, **kw):
    return pkg.make_params(**AR.kw_of(), layout=pkg.SC_SOA if soa else pkg.SC_AOS, **kw)


def _frame(pkg, r, src, tgt, soa=False, **kw):
    """sc_register on (src, tgt): the frame the context then holds -> its result, Rt (12,) with it"""
    a, b = (np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)) if soa else (src, tgt)
    f = r.register(a, b, params=_params(pkg, soa, **kw))
    assert f["status"] == SC_OK
    f["Rt"] = np.concatenate([f["R"].ravel(), f["t"]]).astype(np.float32)
    return f


def _assert_same(got, exp, what=""):
    (gl, gd, gr), (el, ed, er) = got, exp
    print(what, "counts", gr["count"][:8].tolist(), "expected", er["count"][:8].tolist(), "labelled", int((gl >= 0).sum()), int((el >= 0).sum()))
    assert np.array_equal(gl, el), what
    if gd is not None:
        assert gd.view(np.uint32).tobytes() == ed.view(np.uint32).tobytes(), what
    assert gr.tobytes() == er.tobytes(), what


def _device(pkg, r, ap, pose_bytes, stride, k, n, sel=None, want_d2=True):
    """the device form on host data: copies in, one call, one device-wide wait -> (label, d2 or None, records)"""
    import torch
    d_pose = torch.from_numpy(np.frombuffer(pose_bytes, np.uint8).copy()).cuda()
    d_sel = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).cuda()
    d_label = torch.full((n,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
    d_d2 = torch.full((n,), 7.0, dtype=torch.float32, device="cuda") if want_d2 else None
    d_asg = torch.full((k * REC,), 0xAB, dtype=torch.uint8, device="cuda")  # (the call zeroes it itself)
    torch.cuda.synchronize()
    r.assign_poses_frame_device(ap, d_pose.data_ptr(), stride, k, 0 if d_sel is None else d_sel.data_ptr(), d_label.data_ptr(),
                                0 if d_d2 is None else d_d2.data_ptr(), d_asg.data_ptr())
    torch.cuda.synchronize()
    assert d_pose.cpu().numpy().tobytes() == pose_bytes  # d_pose is read, never written
    return (d_label.cpu().numpy(), None if d_d2 is None else d_d2.cpu().numpy(),
            np.frombuffer(d_asg.cpu().numpy().tobytes(), pkg.ASSIGN_RESULT_DTYPE))


def _pose_lists(gt, n):
    """K -> poses: 1, 2, 3 with a duplicate, 64, 65 and — where the reference stays quick — 1024"""
    two = AR.perturbed(gt, 2, 100 + n)
    out = {1: gt[None, :], 2: two, 3: np.stack([two[0], two[1], two[0]]), 64: AR.many(gt, 64, 200 + n), 65: AR.many(gt, 65, 300 + n)}
    if n in (T + 1, 7400):
        out[1024] = AR.many(gt, 1024, 400 + n)
    return out


# ---- the reference, both modes, every pose count; equality 1 ---------------------------------------------------------------------
@pytest.mark.parametrize("n,soa", [(65, False), (129, False), (129, True), (T - 1, False), (T + 1, False), (7400, False)])
def test_labels_residuals_and_records_equal_the_reference(pkg, O, reg, n, soa):
    sc = AR.scene(pkg, n)
    f = _frame(pkg, reg, sc.src, sc.tgt, soa)
    gt = AR.rt_of(sc.R_gt, sc.t_gt)
    for K, poses in _pose_lists(gt, n).items():
        for mode in (AR.BEST, AR.FIRST):
            exp = AR.assign(O, sc.src, sc.tgt, poses, AR.TAU, mode)
            got = reg.assign_poses_frame(poses, mode=mode)
            _assert_same(got, exp, f"n={n} soa={soa} K={K} mode={mode}")
            assert (got[2]["status"] == SC_OK).all() and int(got[2]["count"].sum()) == int((got[0] >= 0).sum())
            assert np.array_equal(got[2]["score"], got[2]["count"])  # the inlier-count mode
        if K in (3, 1024):  # host form == device form, with and without d_d2; the call may be repeated
            ap = pkg.make_assign_params(mode=AR.BEST)
            best = reg.assign_poses_frame(poses)
            dev = _device(pkg, reg, ap, poses.tobytes(), 48, K, n)
            _assert_same(dev, best, f"n={n} K={K} device form")
            nod2 = _device(pkg, reg, ap, poses.tobytes(), 48, K, n, want_d2=False)
            assert np.array_equal(nod2[0], best[0]) and nod2[2].tobytes() == best[2].tobytes()
        if K == 3:
            assert int(best[2]["count"][2]) == 0  # the copy never wins its tie
    # equality 1: one pose, no selection: label + 1 is sc_mask_host's mask and count is the restatement's score — for the frame's own
    # winner, and for a hostile finite pose whose residual is inf or NaN
    a, b = (np.ascontiguousarray(sc.src.T), np.ascontiguousarray(sc.tgt.T)) if soa else (sc.src, sc.tgt)
    for name, Rt in (("winner", f["Rt"]), ("hostile", AR.hostile())):
        for mode in (AR.BEST, AR.FIRST):
            lab, d2, rec = reg.assign_poses_frame(Rt, mode=mode)
            count = int(O.score(sc.src, sc.tgt, Rt[None, :], AR.TAU)[0])
            print(name, mode, int(rec[0]["count"]), count)
            assert int(rec[0]["status"]) == SC_OK and int(rec[0]["count"]) == count == int(rec[0]["score"])
            assert np.array_equal((lab + 1).astype(np.uint8), O.mask(sc.src, sc.tgt, Rt, AR.TAU))
        assert (name == "winner") == (count >= 3)
    lab = reg.assign_poses_frame(f["Rt"])[0]
    assert np.array_equal((lab + 1).astype(np.uint8), reg.mask(a, b, _params(pkg, soa), f["Rt"]))


# ---- equality 2: FIRST on the motions of sc_register_instances returns its label and its scores --------------------------------------
@pytest.mark.parametrize("score_mode", (0,) + CONFIRMED_SCORE_MODES)
def test_first_on_the_instances_motions_returns_their_label_and_scores(pkg, O, reg, score_mode):
    mo = AR.motions(pkg)
    min_score = 20 if score_mode == 0 else 20 * 1024
    inst = reg.register_instances(mo.src, mo.tgt, max_instances=4, min_score=min_score, params=_params(pkg, score_mode=score_mode))
    K = len(inst["Rt"])
    print("motions", K, "scores", inst["score"].tolist())
    assert inst["status"] == SC_OK and K >= 2
    got = reg.assign_poses_frame(inst["Rt"], mode=AR.FIRST)  # stride 48, no flag
    _assert_same(got, AR.assign(O, mo.src, mo.tgt, inst["Rt"], AR.TAU, AR.FIRST, score_mode=score_mode), f"score_mode {score_mode}")
    assert np.array_equal(got[0], inst["label"])
    assert got[2]["score"].tolist() == inst["score"].tolist()
    if score_mode == 0:
        assert np.array_equal(got[2]["count"], inst["score"])
    # BEST on the same motions scores in the same mode
    _assert_same(reg.assign_poses_frame(inst["Rt"]), AR.assign(O, mo.src, mo.tgt, inst["Rt"], AR.TAU, AR.BEST, score_mode=score_mode), "BEST")


# ---- equalities 3 and 4: the information matrix under the labels; two rounds of the device-side loop ---------------------------------
def test_pose_info_under_the_labels_counts_what_was_assigned(pkg, O, reg):
    import torch
    n = 7400
    sc = AR.scene(pkg, n)
    _frame(pkg, reg, sc.src, sc.tgt)
    poses = AR.many(AR.rt_of(sc.R_gt, sc.t_gt), 16, 5)
    K = len(poses)
    d_pose = torch.from_numpy(poses).cuda()
    d_label = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_asg = torch.zeros(K * REC, dtype=torch.uint8, device="cuda"); d_info = torch.zeros(K * 320, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reg.assign_poses_frame_device(pkg.make_assign_params(), d_pose.data_ptr(), 48, K, 0, d_label.data_ptr(), 0, d_asg.data_ptr())
    reg.pose_info_frame_device(pkg.make_pose_info_params(sel_mode=pkg.SC_POSE_INFO_SEL_LABEL), d_pose.data_ptr(), 48, K, d_label.data_ptr(),
                               d_info.data_ptr())
    torch.cuda.synchronize()
    asg = np.frombuffer(d_asg.cpu().numpy().tobytes(), pkg.ASSIGN_RESULT_DTYPE)
    info = np.frombuffer(d_info.cpu().numpy().tobytes(), pkg.POSE_INFO_RESULT_DTYPE)
    print(asg["count"].tolist())
    assert np.array_equal(info["inliers"], asg["count"]) and (asg["count"] > 0).sum() >= 8 and int(asg["count"].sum()) == int((d_label.cpu().numpy() >= 0).sum())


def test_two_rounds_of_the_device_side_loop_equal_the_references(pkg, O, reg):
    """sc_register_instances -> sc_polish_poses_device(SEL_ALIVE) -> [sc_assign_poses_frame_device(BEST) ->
    sc_polish_poses_device(SEL_LABEL, max_iter = 1)] x 2 -> sc_pose_info_frame_device(SEL_LABEL), one wait at the end."""
    import torch
    mo = AR.motions(pkg)
    n = len(mo.src)
    inst = reg.register_instances(mo.src, mo.tgt, max_instances=4, min_score=20, params=_params(pkg))
    K = len(inst["Rt"])
    assert inst["status"] == SC_OK and K >= 2
    d_rt = torch.from_numpy(inst["Rt"]).cuda(); d_lab0 = torch.from_numpy(inst["label"]).cuda()
    d_pol = [torch.zeros(K * 64, dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_label = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_asg = [torch.zeros(K * REC, dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_info = torch.zeros(K * 320, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    PP, ST = pkg.make_polish_poses_params, pkg.SC_POLISH_POSES_STATUS
    reg.polish_poses_device(PP(sel_mode=pkg.SC_POLISH_POSES_SEL_ALIVE), d_rt.data_ptr(), 48, K, d_lab0.data_ptr(), d_pol[0].data_ptr(), 0)
    for i in range(2):
        reg.assign_poses_frame_device(pkg.make_assign_params(flags=pkg.SC_ASSIGN_STATUS), d_pol[i].data_ptr(), 64, K, 0, d_label[i].data_ptr(), 0,
                                      d_asg[i].data_ptr())
        reg.polish_poses_device(PP(max_iter=1, sel_mode=pkg.SC_POLISH_POSES_SEL_LABEL, flags=ST), d_pol[i].data_ptr(), 64, K, d_label[i].data_ptr(),
                                d_pol[i + 1].data_ptr(), 0)
    reg.pose_info_frame_device(pkg.make_pose_info_params(sel_mode=pkg.SC_POSE_INFO_SEL_LABEL, flags=pkg.SC_POSE_INFO_STATUS), d_pol[2].data_ptr(), 64,
                               K, d_label[1].data_ptr(), d_info.data_ptr())
    torch.cuda.synchronize()
    # the same loop on the references
    pol = PF.poses(O, mo.src, mo.tgt, inst["Rt"], AR.TAU, PF.SEL_ALIVE, inst["label"])[0]
    assert d_pol[0].cpu().numpy().tobytes() == pol.tobytes()
    for i in range(2):
        lab, _, asg = AR.assign(O, mo.src, mo.tgt, pol["Rt"], AR.TAU, AR.BEST, statuses=pol["status"])
        assert np.array_equal(d_label[i].cpu().numpy(), lab), i
        assert d_asg[i].cpu().numpy().tobytes() == asg.tobytes(), i
        pol = PF.poses(O, mo.src, mo.tgt, pol["Rt"], AR.TAU, PF.SEL_LABEL, lab, statuses=pol["status"], max_iter=1)[0]
        assert d_pol[i + 1].cpu().numpy().tobytes() == pol.tobytes(), i
        print("round", i, asg["count"].tolist(), "moved from the greedy label:", int((lab != inst["label"]).sum()))
    info = PIF.frame(O, mo.src, mo.tgt, pol["Rt"], AR.TAU, PIF.SEL_LABEL, lab, statuses=pol["status"])
    assert d_info.cpu().numpy().tobytes() == info.tobytes()
    assert (lab != inst["label"]).any()  # the relabel did something the greedy label had not


# ---- 5: SEL_MASK; 6: statuses ------------------------------------------------------------------------------------------------------------
def test_the_byte_mask_and_the_statuses(pkg, O, reg):
    mo = AR.motions(pkg)
    n = len(mo.src)
    _frame(pkg, reg, mo.src, mo.tgt)
    poses = np.stack([AR.rt_of(R, t) for R, t in mo.motions] + [AR.perturbed(AR.rt_of(*mo.motions[0]), 1, 8)[0]])
    sel = (np.arange(n) % 3 != 0).astype(np.uint8) * 5  # (any non-zero byte)
    for mode in (AR.BEST, AR.FIRST):
        got = reg.assign_poses_frame(poses, mode=mode, sel_mode=pkg.SC_ASSIGN_SEL_MASK, sel=sel)
        _assert_same(got, AR.assign(O, mo.src, mo.tgt, poses, AR.TAU, mode, sel), f"mask, mode {mode}")
        assert (got[0][sel == 0] == -1).all() and (got[1][sel == 0].view(np.uint32) == 0x7F800000).all() and (got[0][sel != 0] >= 0).sum() > 300
        rows = AR.assign(O, mo.src[sel != 0], mo.tgt[sel != 0], poses, AR.TAU, mode)
        assert got[2].tobytes() == rows[2].tobytes() and np.array_equal(got[0][sel != 0], rows[0])  # the records are those of the selected rows
        dev = _device(pkg, reg, pkg.make_assign_params(mode=mode, sel_mode=pkg.SC_ASSIGN_SEL_MASK), poses.tobytes(), 48, 3, n, sel)
        _assert_same(dev, got, "mask, device form")
    nothing = reg.assign_poses_frame(poses, sel_mode=pkg.SC_ASSIGN_SEL_MASK, sel=np.zeros(n, np.uint8))
    assert (nothing[0] == -1).all() and not nothing[2]["count"].any() and (nothing[2]["status"] == SC_OK).all()
    # with SEL_NONE a selection that is given is not read
    assert np.array_equal(reg.assign_poses_frame(poses, sel=np.zeros(n, np.uint8))[0], reg.assign_poses_frame(poses)[0])
    # statuses: a status other than SC_OK and a non-finite Rt among good poses change only their own record and claim nothing
    goods = {mode: reg.assign_poses_frame(poses[:2], mode=mode) for mode in (AR.BEST, AR.FIRST)}
    for dt in (pkg.BATCH_RESULT_DTYPE, pkg.api.POLISH_BATCH_RESULT_DTYPE):  # stride 80 and stride 64
        pose = np.zeros(6, dt)
        pose["Rt"] = [poses[1], poses[0], poses[1], poses[0], poses[1], poses[1]]
        pose["status"] = [SC_ENOHYP, SC_OK, 77, SC_OK, SC_OK, SC_OK]
        pose["Rt"][3][7] = np.nan
        pose["Rt"][4][11] = np.inf
        for mode in (AR.BEST, AR.FIRST):
            got, good = reg.assign_poses_frame(pose, mode=mode, flags=pkg.SC_ASSIGN_STATUS), goods[mode]
            _assert_same(got, AR.assign(O, mo.src, mo.tgt, pose["Rt"], AR.TAU, mode, statuses=pose["status"]), f"stride {dt.itemsize}, the flag")
            assert got[2]["status"].tolist() == [SC_ENOHYP, SC_OK, 77, SC_EINVAL, SC_EINVAL, SC_OK]
            assert not got[2]["count"][[0, 2, 3, 4]].any() and not got[2]["score"][[0, 2, 3, 4]].any() and not got[2]["reserved"].any()
            assert np.array_equal(np.where(got[0] == 1, 0, np.where(got[0] == 5, 1, got[0])), good[0]) and got[1].tobytes() == good[1].tobytes()
            assert got[2]["count"][[1, 5]].tolist() == good[2]["count"].tolist()
        dev = _device(pkg, reg, pkg.make_assign_params(flags=pkg.SC_ASSIGN_STATUS), pose.tobytes(), dt.itemsize, 6, n)
        _assert_same(dev, reg.assign_poses_frame(pose, flags=pkg.SC_ASSIGN_STATUS), "statuses, device form")
        # without the flag byte 48 is not read: poses 0 and 2 are poses like any other
        plain = reg.assign_poses_frame(pose)
        _assert_same(plain, AR.assign(O, mo.src, mo.tgt, pose["Rt"], AR.TAU), f"stride {dt.itemsize}, no flag")
        assert plain[2]["status"].tolist() == [SC_OK, SC_OK, SC_OK, SC_EINVAL, SC_EINVAL, SC_OK] and int(plain[2]["count"][0]) > 0
    # ... and so is the rank of an sc_polish_cand record (stride 64, no flag)
    pol = reg.polish(candidates=4, max_iter=2)
    assert pol["n_cand"] == 4 and (pol["cand"]["rank"] != 0).any()
    _assert_same(reg.assign_poses_frame(pol["cand"]), AR.assign(O, mo.src, mo.tgt, pol["cand"]["Rt"], AR.TAU), "cand records, no flag")


# ---- 7: scale ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [40, -40])
def test_scaled_frames_give_the_same_labels_and_counts(pkg, O, reg, k):
    """the coordinates, tau and the translations times 2^k: every residual is the unscaled one times 2^2k exactly while it stays normal
    (tests/test_range_oracle.py: k lies inside the windows of C2 and of the whole path), so every comparison falls the same way"""
    assert in_window(k, WIN_C2) and in_window(k, WIN_REGISTER)
    n = T + 1
    sc = AR.scene(pkg, n)
    poses = AR.many(AR.rt_of(sc.R_gt, sc.t_gt), 16, 6)
    _frame(pkg, reg, sc.src, sc.tgt)
    base = {mode: reg.assign_poses_frame(poses, mode=mode) for mode in (AR.BEST, AR.FIRST)}
    src, tgt = scaled(sc.src, k), scaled(sc.tgt, k)
    pk = poses.copy(); pk[:, 9:] = scaled(poses[:, 9:], k)
    kw = scaled_kw(k, base={x: AR.kw_of()[x] for x in ("sigma", "t_cmp", "tau", "min_len")}, max_triangles=AR.kw_of()["max_triangles"])
    f = reg.register(src, tgt, params=pkg.make_params(**kw))
    assert f["status"] == SC_OK
    for mode in (AR.BEST, AR.FIRST):
        lab, d2, rec = reg.assign_poses_frame(pk, mode=mode)
        assert np.array_equal(lab, base[mode][0]) and rec.tobytes() == base[mode][2].tobytes() and int(rec["count"].sum()) > 100
        with np.errstate(over="ignore"):
            want = np.where(base[mode][0] >= 0, base[mode][1] * pow2(k) * pow2(k), np.float32(np.inf)).astype(np.float32)
        assert d2.tobytes() == want.tobytes()
        _assert_same((lab, d2, rec), AR.assign(O, src, tgt, pk, kw["tau"], mode), f"k={k} mode={mode}")


# ---- 8: the frame is untouched -------------------------------------------------------------------------------------------------------
def _flat(res):
    return dict(status=res["status"], Rt=np.concatenate([res["R"].ravel(), res["t"]]).astype(np.float32), mask=res["mask"],
                stats={k: res["stats"][k] for k in STAT_KEYS})


def _same(a, b, what):
    assert a["status"] == b["status"] and np.array_equal(a["mask"], b["mask"]) and a["Rt"].tobytes() == b["Rt"].tobytes(), what
    assert a["stats"] == b["stats"], what


def test_the_frame_stays_untouched_and_usable(pkg, O):
    mo = AR.motions(pkg)
    with_call, without = pkg.Registrar(0), pkg.Registrar(0)
    try:
        f = _frame(pkg, with_call, mo.src, mo.tgt)
        _frame(pkg, without, mo.src, mo.tgt)
        poses = np.stack([f["Rt"], AR.rt_of(*mo.motions[1])])
        exp = AR.assign(O, mo.src, mo.tgt, poses, AR.TAU)
        _assert_same(with_call.assign_poses_frame(poses), exp, "before the round")
        r1 = _flat(with_call.peel())
        _same(r1, _flat(without.peel()), "round 1")
        assert r1["status"] == SC_OK
        _assert_same(with_call.assign_poses_frame(poses, mode=AR.FIRST), AR.assign(O, mo.src, mo.tgt, poses, AR.TAU, AR.FIRST), "between the rounds")
        _same(_flat(with_call.peel()), _flat(without.peel()), "round 2")
        pa, pb = with_call.polish(candidates=4, max_iter=8), without.polish(candidates=4, max_iter=8)
        _same(_flat(pa), _flat(pb), "polish")
        assert pa["n_cand"] == pb["n_cand"] and pa["cand"].tobytes() == pb["cand"].tobytes()
        assert with_call.pose_info_frame(poses).tobytes() == without.pose_info_frame(poses).tobytes()
        a, b = with_call.polish_poses(poses), without.polish_poses(poses)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
        _assert_same(with_call.assign_poses_frame(poses), exp, "after everything")
    finally:
        with_call.close(); without.close()


# ---- 9: what is refused, and what a refused call leaves --------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_frame(pkg, O):
    import torch
    L = pkg.load_library()
    sc = AR.scene(pkg, 129)
    r = pkg.Registrar(0)
    try:
        pose = np.zeros(2, pkg.BATCH_RESULT_DTYPE)
        label = np.zeros(129, np.int32); d2 = np.zeros(129, np.float32); asg = np.zeros(2, AR.RESULT_DTYPE)
        sel = np.ones(129, np.uint8)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

        def call(ap, stride=80, k=2, sel=None, pose=pose, label=label, asg=asg, entry=L.sc_assign_poses_frame):
            rc = entry(r._h, None if ap is None else C.byref(ap), vp(pose), stride, k, vp(sel), vp(label), vp(d2), vp(asg))
            return rc, L.sc_last_error(r._h).decode()

        ok = pkg.make_assign_params()
        rc, text = call(ok)  # no frame on a fresh context
        assert rc == SC_EINVAL and "no frame" in text and "sc_assign_poses_frame" in text
        f = _frame(pkg, r, sc.src, sc.tgt)
        pose["Rt"], pose["status"] = f["Rt"], SC_OK
        good = r.assign_poses_frame(pose)
        _assert_same(good, AR.assign(O, sc.src, sc.tgt, pose["Rt"], AR.TAU), "good")
        short = pkg.make_assign_params(); short.size = 28
        res = pkg.make_assign_params(); res.reserved[3] = 1
        mk = pkg.make_assign_params
        cases = {
            "ap NULL": (lambda: call(None), "NULL"),
            "pose NULL": (lambda: call(ok, pose=None), "NULL"),
            "label NULL": (lambda: call(ok, label=None), "NULL"),
            "asg NULL": (lambda: call(ok, asg=None), "NULL"),
            "size": (lambda: call(short), "size"),
            "mode 2": (lambda: call(mk(mode=2)), "mode"),
            "sel_mode 2": (lambda: call(mk(sel_mode=2), sel=sel), "sel_mode"),
            "mask without sel": (lambda: call(mk(sel_mode=1)), "sel is NULL"),
            "flag 2": (lambda: call(mk(flags=2)), "flag"),
            "flag 3": (lambda: call(mk(flags=3)), "flag"),
            "reserved": (lambda: call(res), "reserved"),
            "n_poses 0": (lambda: call(ok, k=0), "n_poses"),
            "n_poses 1025": (lambda: call(ok, k=1025), "n_poses"),
            "stride 0": (lambda: call(ok, stride=0), "pose_stride"),
            "stride 44": (lambda: call(ok, stride=44), "pose_stride"),
            "stride 50": (lambda: call(ok, stride=50), "pose_stride"),
            "stride 48 with the flag": (lambda: call(mk(flags=1), stride=48), "pose_stride"),
            "device form, stride 50": (lambda: call(ok, stride=50, entry=L.sc_assign_poses_frame_device), "sc_assign_poses_frame_device"),
        }
        for what, (fn, word) in cases.items():
            rc, text = fn()
            print(what, rc, text)
            assert rc == SC_EINVAL and word in text and "sc_assign_poses_frame" in text, what
            _assert_same(r.assign_poses_frame(pose), good, what)  # the refused call left the context and the frame
        assert L.sc_assign_poses_frame(None, C.byref(ok), vp(pose), 80, 2, None, vp(label), None, vp(asg)) == SC_EINVAL
        assert call(mk(sel_mode=1), sel=sel)[0] == SC_OK
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
        r._frame_n = 129
        _assert_same(r.assign_poses_frame(pose), good, "after the async frame")  # no output depends on how the frame was enqueued
    finally:
        r.close()


# ---- 10: the workspace: allocated by the first call, held against the frame's cap --------------------------------------------------------
def test_workspace_appears_with_the_first_call_and_respects_the_cap(pkg, O):
    n = 7400
    sc = AR.scene(pkg, n)
    r = pkg.Registrar(0)
    try:
        r.set_debug(no_fast=1)  # (the same input takes the same path every time: what moves afterwards is these entries')
        p = _params(pkg)
        held = [r.register(sc.src, sc.tgt, params=p)["stats"]["workspace_bytes"] for _ in range(4)]
        assert held[2] == held[3] > 0, held
        f = _frame(pkg, r, sc.src, sc.tgt)
        poses = np.tile(f["Rt"], (64, 1))
        got = r.assign_poses_frame(poses)
        assert r.peel()["status"] in (SC_OK, SC_ENOHYP)  # (the rounds' own workspace exists from here on)
        after = r.register(sc.src, sc.tgt, params=p)["stats"]["workspace_bytes"]
        print(held, after)
        assert after >= held[3] + 64 * 48 + 2 * n * 4 + 64 * REC  # the host form's copies: poses, labels, residuals, records
        again = r.assign_poses_frame(poses)
        _assert_same(again, got, "again")
        assert r.register(sc.src, sc.tgt, params=p)["stats"]["workspace_bytes"] == after
        assert int(got[2]["count"][0]) == f["stats"]["best_count"] and not got[2]["count"][1:].any()  # 63 copies claim nothing
        # the device form allocates nothing: the tallies are added into the caller's records
        dev = _device(pkg, r, pkg.make_assign_params(), np.tile(f["Rt"], (1024, 1)).tobytes(), 48, 1024, n)
        assert np.array_equal(dev[0], got[0]) and r.register(sc.src, sc.tgt, params=p)["stats"]["workspace_bytes"] == after
        # a cap with no room for the host form's copies: SC_ENOMEM, nothing enqueued, the context and the frame stay usable
        fc = _frame(pkg, r, sc.src, sc.tgt, max_workspace=after + 4096)
        assert fc["Rt"].tobytes() == f["Rt"].tobytes()
        wide = np.zeros(1024, np.dtype([("Rt", np.float32, 12), ("pad", np.uint8, 976)]))  # stride 1024: a MiB of pose records
        wide["Rt"] = f["Rt"]
        with pytest.raises(pkg.SacCotError) as e:
            r.assign_poses_frame(wide)
        assert e.value.status == SC_ENOMEM
        _assert_same(r.assign_poses_frame(poses), got, "what fits still runs")
        assert r.peel()["status"] in (SC_OK, SC_ENOHYP)  # ... and so does a round
    finally:
        r.close()
