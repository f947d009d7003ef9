"""GPU: poses relabelled and refitted until stable for a batch's problems (include/saccot.h, sc_settle_poses_batch /
sc_settle_poses_batch_device).

The expected value of every case is tests/settle_ref.py per problem, and every comparison is bit for bit: the 64 bytes of every
record, every label, both words of every problem's d_rounds.  GPU against GPU as well: the frame form on the same problem (equality
3 of the header), the planes of sc_register_instances_batch_device as the input, and the device form against the host form.
"""
import numpy as np
import pytest

import instances_batch_ref as IB
import settle_ref as SR

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
SIZES = ((3, 1.0), (64, .4), (65, .4), (512, .3))  # (n, rho): the smallest problem, one bit word and a bit, the maximum
REC = 64


def _params(pkg, soa=False, **kw):
    return pkg.make_params(**SR.kw_of(), layout=pkg.SC_SOA if soa else pkg.SC_AOS, **kw)


def _scenes(pkg):
    return [pkg.synth.make_scene(n, rho, 1.0, SR.TAU, 7600 + n) for n, rho in SIZES]


def _pack(scenes, soa=False):
    src, tgt = np.concatenate([s.src for s in scenes]), np.concatenate([s.tgt for s in scenes])
    offset = np.concatenate([[0], np.cumsum([len(s.src) for s in scenes])]).astype(np.uint32)
    if soa:
        src, tgt = np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)
    return src, tgt, offset


def _poses(pkg, scenes, K, dtype=None):
    """(K, B) pose records, motion-major: starts a fraction of tau away from every problem's own motion (a few rounds to settle), for
    K = 16 neighbours, far poses and a copy (assign_ref.many) with a plane of SC_ENOHYP and a non-finite pose among them"""
    pose = np.zeros((K, len(scenes)), dtype or pkg.BATCH_RESULT_DTYPE)
    for b, s in enumerate(scenes):
        gt = SR.rt_of(s.R_gt, s.t_gt)
        pose["Rt"][:, b] = SR.many(gt, K, 500 + b) if K > 2 else SR.perturbed(gt, K, 9 + b, 1e-2, 2e-2)
    if K >= 16:
        pose["status"][2, :] = SC_ENOHYP
        pose["Rt"][4, 1][5] = np.nan
    return pose


def _assert_batch(got, exp, offset, what=""):
    (gr, gl, gn), (er, el, en) = got, exp
    for b in range(len(offset) - 1):
        lo, hi = int(offset[b]), int(offset[b + 1])
        print(what, "problem", b, "rounds", gn[b].tolist(), "expected", en[b].tolist(), "scores", gr["score"][:6, b].tolist(), er["score"][:6, b].tolist())
        assert gn[b].tolist() == en[b].tolist(), (what, b)
        assert np.array_equal(gl[lo:hi], el[b]), (what, b)
        assert np.ascontiguousarray(gr[:, b]).tobytes() == np.ascontiguousarray(er[:, b]).tobytes(), (what, b)


@pytest.mark.parametrize("K,soa,max_iter", [(1, False, 16), (2, False, 16), (2, True, 2), (16, False, 16), (16, True, 1)])
def test_the_batch_equals_the_reference_and_the_frame_form(pkg, O, reg, K, soa, max_iter):
    scenes = _scenes(pkg)
    problems = [(s.src, s.tgt) for s in scenes]
    src, tgt, offset = _pack(scenes, soa)
    p = _params(pkg, soa)
    pose = _poses(pkg, scenes, K)
    got = reg.settle_poses_batch(src, tgt, offset, p, pose, max_iter=max_iter)
    exp = SR.batch(O, problems, pose["Rt"], SR.TAU, pose["status"], max_iter=max_iter)
    _assert_batch(got, exp, offset, f"K={K} soa={soa} max_iter={max_iter}")
    if max_iter == 16:
        assert (got[2][1:, 0] >= 1).all()  # the starts were not fixed points: rounds were counted
    if K >= 16:
        assert (got[0]["status"][2] == SC_ENOHYP).all() and int(got[0]["status"][4, 1]) == SC_EINVAL
        assert not got[0]["score"][2].any() and (got[0]["stop"][2] == SR.STOP_DECLINED).all()
    if not soa:  # the device form, stride 64 (sc_polish_batch_result), outputs pre-filled with sentinel bytes: the same bytes
        import torch
        pose64 = _poses(pkg, scenes, K, pkg.api.POLISH_BATCH_RESULT_DTYPE)
        B = len(scenes)
        d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
        d_pose = torch.from_numpy(pose64.view(np.uint8).reshape(-1).copy()).cuda()
        d_pol = torch.full((K * B * REC,), 0xAB, dtype=torch.uint8, device="cuda")
        d_label = torch.full((int(offset[-1]),), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
        d_rounds = torch.full((2 * B,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sp = pkg.make_settle_params(max_iter=max_iter)
        reg.settle_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, sp, d_pose.data_ptr(), 64, K, d_pol.data_ptr(),
                                      d_label.data_ptr(), d_rounds.data_ptr())
        torch.cuda.synchronize()
        assert d_pol.cpu().numpy().tobytes() == got[0].tobytes() and np.array_equal(d_label.cpu().numpy(), got[1])
        assert d_rounds.cpu().numpy().view(np.uint32).tobytes() == got[2].tobytes()
        assert d_pose.cpu().numpy().tobytes() == pose64.tobytes()  # d_pose is read, never written
        d_label.fill_(0x2B2B2B2B); d_pol.fill_(0xAB)
        torch.cuda.synchronize()
        reg.settle_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, sp, d_pose.data_ptr(), 64, K, d_pol.data_ptr(),
                                      d_label.data_ptr(), 0)  # d_rounds NULL
        torch.cuda.synchronize()
        assert d_pol.cpu().numpy().tobytes() == got[0].tobytes() and np.array_equal(d_label.cpu().numpy(), got[1])
    # equality 3: the frame form on the same problem (the batch call above ended every frame, so each problem is registered first)
    # AoS and SoA batches alike (the frame is registered from the n x 3 arrays either way), so max_iter 16, 2 and 1 are all covered
    if K in (2, 16):
        framed = 0
        for b, s in enumerate(scenes):
            if reg.register(s.src, s.tgt, params=_params(pkg))["status"] != SC_OK:
                # SC_ENOHYP leaves no frame.  Only problem 0 — three correspondences, which may hold no triangle — may go that way:
                # a frame lost for any other size is a failure, not a skipped comparison
                assert b == 0, f"problem {b} (n = {len(s.src)}) left no frame"
                continue
            framed += 1
            lo, hi = int(offset[b]), int(offset[b + 1])
            rec, lab, _, rounds = reg.settle_poses_frame(np.ascontiguousarray(pose[:, b]), max_iter=max_iter, flags=pkg.SC_SETTLE_STATUS)
            assert np.array_equal(lab, got[1][lo:hi]) and rounds.tolist() == got[2][b].tolist(), b
            assert rec.tobytes() == np.ascontiguousarray(got[0][:, b]).tobytes(), b
        assert framed >= 3


def test_the_planes_of_the_instances_batch_settle(pkg, O, reg):
    """sc_register_instances_batch_device's d_res, stride 80, planes past nfound SC_ENOHYP, straight into the settle call on the
    same stream: no wait between the two"""
    import torch
    problems = IB.scenes(pkg)
    B, K = len(problems), 4
    src, tgt = np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems])
    offset = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.uint32)
    total = int(offset[-1])
    p = pkg.make_params(**IB.KW, max_triangles=SR.kw_of()["max_triangles"])
    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    d_res = torch.zeros(K * B * 80, dtype=torch.uint8, device="cuda")
    d_label = torch.zeros(total, dtype=torch.int32, device="cuda"); d_nfound = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_lab2 = torch.full((total,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
    d_pol = torch.full((K * B * REC,), 0xAB, dtype=torch.uint8, device="cuda")
    d_rounds = torch.full((2 * B,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    reg.register_instances_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, K, 3, d_res.data_ptr(), d_label.data_ptr(),
                                        d_nfound.data_ptr())
    reg.settle_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, pkg.make_settle_params(), d_res.data_ptr(), 80, K,
                                  d_pol.data_ptr(), d_lab2.data_ptr(), d_rounds.data_ptr())
    torch.cuda.synchronize()
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE).reshape(K, B)
    pol = np.frombuffer(d_pol.cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE).reshape(K, B)
    rounds = d_rounds.cpu().numpy().view(np.uint32).reshape(B, 2)
    nfound = d_nfound.cpu().numpy()
    print("nfound", nfound.tolist(), "rounds", rounds.tolist(), "scores", pol["score"].T.tolist())
    assert nfound.max() >= 2 and (rounds[:, 0] >= 1).any()
    exp = SR.batch(O, problems, res["Rt"], IB.KW["tau"], res["status"])
    _assert_batch((pol, d_lab2.cpu().numpy(), rounds), exp, offset, "instances planes")
    for b in range(B):
        for k in range(K):
            assert (int(pol[k, b]["status"]) == SC_OK) == (k < nfound[b])  # a plane without a motion is passed through
    assert (d_lab2.cpu().numpy() != d_label.cpu().numpy()).any()  # the settled labels repair the greedy ones


def test_a_nan_coordinate_is_einval_alone_and_position_does_not_matter(pkg, O, reg):
    scenes = _scenes(pkg)
    K = 16
    pose = _poses(pkg, scenes, K)
    p = _params(pkg)
    src, tgt, offset = _pack(scenes)
    clean = reg.settle_poses_batch(src, tgt, offset, p, pose, max_iter=4)
    bad_tgt = tgt.copy(); bad_tgt[int(offset[2]) + 7, 1] = np.nan  # problem 2
    rec, lab, rounds = reg.settle_poses_batch(src, bad_tgt, offset, p, pose, max_iter=4)
    lo, hi = int(offset[2]), int(offset[3])
    assert (lab[lo:hi] == -1).all() and (rec["status"][:, 2] == SC_EINVAL).all() and not rec["score"][:, 2].any()
    assert rounds[2].tolist() == [0, SR.STOP_DECLINED] and (rec["stop"][:, 2] == SR.STOP_DECLINED).all()
    keep = np.ones(len(lab), bool); keep[lo:hi] = False
    assert np.array_equal(lab[keep], clean[1][keep])
    for b in (0, 1, 3):
        assert np.ascontiguousarray(rec[:, b]).tobytes() == np.ascontiguousarray(clean[0][:, b]).tobytes() and rounds[b].tolist() == clean[2][b].tolist()
    problems = [(s.src, s.tgt) for s in scenes]
    problems[2] = (scenes[2].src, bad_tgt[lo:hi])
    _assert_batch((rec, lab, rounds), SR.batch(O, problems, pose["Rt"], SR.TAU, pose["status"], max_iter=4), offset, "a NaN in problem 2")
    # position independence: problem 3 first, last and alone, in batches of 6, 2 and 1 problems: the same bytes
    order = [3, 0, 1, 2, 1, 3]
    s6, t6, o6 = _pack([scenes[b] for b in order])
    r6, l6, n6 = reg.settle_poses_batch(s6, t6, o6, p, np.ascontiguousarray(pose[:, order]), max_iter=4)
    for pos, b in enumerate(order):
        assert np.array_equal(l6[int(o6[pos]): int(o6[pos + 1])], clean[1][int(offset[b]): int(offset[b + 1])]), pos
        assert np.ascontiguousarray(r6[:, pos]).tobytes() == np.ascontiguousarray(clean[0][:, b]).tobytes() and n6[pos].tolist() == clean[2][b].tolist(), pos
    s1, t1, o1 = _pack([scenes[3]])
    r1, l1, n1 = reg.settle_poses_batch(s1, t1, o1, p, np.ascontiguousarray(pose[:, 3:4]), max_iter=4)
    assert np.array_equal(l1, clean[1][int(offset[3]):]) and r1.tobytes() == np.ascontiguousarray(clean[0][:, 3:4]).tobytes()


def test_refusals_and_the_entry_ends_the_frame(pkg, O):
    scenes = _scenes(pkg)
    src, tgt, offset = _pack(scenes)
    r = pkg.Registrar(0)
    try:
        p = _params(pkg)
        pose = _poses(pkg, scenes, 2)
        for what, kw, word in (("max_iter 0", dict(max_iter=0), "max_iter"), ("max_iter 65", dict(max_iter=65), "max_iter"),
                               ("a mask", dict(sel_mode=1), "sel_mode"), ("flag 2", dict(flags=2), "flag")):
            with pytest.raises(pkg.SacCotError) as e:
                r.settle_poses_batch(src, tgt, offset, p, pose, **kw)
            print(what, e.value)
            assert e.value.status == SC_EINVAL and word in str(e.value) and "sc_settle_poses_batch" in str(e.value), what
        with pytest.raises(pkg.SacCotError) as e:
            r.settle_poses_batch(src, tgt, offset, p, _poses(pkg, scenes, 17))
        assert e.value.status == SC_EINVAL and "n_poses" in str(e.value)
        with pytest.raises(pkg.SacCotError) as e:
            r.settle_poses_batch(src, tgt, np.array([0, 2], np.uint32), p, pose[:, :1])  # a problem of two correspondences
        assert e.value.status == SC_EINVAL
        s = scenes[3]
        assert r.register(s.src, s.tgt, params=p)["status"] == SC_OK
        r.settle_poses_batch(src, tgt, offset, p, pose)
        r._frame_n = len(s.src)
        with pytest.raises(pkg.SacCotError) as e:
            r.settle_poses_frame(pose["Rt"][:, 3])
        assert e.value.status == SC_EINVAL and "no frame" in str(e.value)
        # a call outstanding on the context: refused until sc_wait, then the same bytes as before
        import torch
        before = r.settle_poses_batch(src, tgt, offset, p, pose)
        n = len(s.src)
        ds, dt = torch.from_numpy(s.src).cuda(), torch.from_numpy(s.tgt).cuda()
        d_Rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
        r.register_device_async(ds.data_ptr(), dt.data_ptr(), n, p, d_Rt.data_ptr(), d_mask.data_ptr())
        with pytest.raises(pkg.SacCotError) as e:
            r.settle_poses_batch(src, tgt, offset, p, pose)
        assert e.value.status == SC_EINVAL and "outstanding" in str(e.value)
        assert r.wait()[0] == SC_OK
        after = r.settle_poses_batch(src, tgt, offset, p, pose)
        assert after[0].tobytes() == before[0].tobytes() and np.array_equal(after[1], before[1]) and after[2].tobytes() == before[2].tobytes()
    finally:
        r.close()
