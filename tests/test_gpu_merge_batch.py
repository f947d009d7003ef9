"""GPU: duplicate poses found and folded for a batch's problems (include/saccot.h, sc_merge_poses_batch /
sc_merge_poses_batch_device).

The expected value of every case is tests/merge_ref.py per problem, and every comparison is bit for bit: the 64 bytes of every
record, every parent, both count words of every problem.  GPU against GPU as well: the frame form on the same problem (equality 4
of the header), the planes of sc_register_instances_batch_device plus perturbed copies as the input, and the device form against the
host form.
"""
import numpy as np
import pytest

import instances_batch_ref as IB
import merge_ref as MR

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
SIZES = ((3, 1.0), (64, .4), (65, .4), (512, .3))  # (n, rho): the smallest problem, one bit word, one and a bit, the maximum
REC = 64


def _params(pkg, soa=False, **kw):
    return pkg.make_params(**MR.kw_of(), layout=pkg.SC_SOA if soa else pkg.SC_AOS, **kw)


def _scenes(pkg):
    return [pkg.synth.make_scene(n, rho, 1.0, MR.TAU, 7600 + n) for n, rho in SIZES]


def _pack(scenes, soa=False):
    src, tgt = np.concatenate([s.src for s in scenes]), np.concatenate([s.tgt for s in scenes])
    offset = np.concatenate([[0], np.cumsum([len(s.src) for s in scenes])]).astype(np.uint32)
    if soa:
        src, tgt = np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)
    return src, tgt, offset


def _poses(pkg, scenes, K, dtype=None):
    """(K, B) pose records, motion-major: neighbours of every problem's own motion, from K = 16 on far poses and an exact copy
    (assign_ref.many) with a plane of SC_ENOHYP and a non-finite pose among them"""
    pose = np.zeros((K, len(scenes)), dtype or pkg.BATCH_RESULT_DTYPE)
    for b, s in enumerate(scenes):
        gt = MR.rt_of(s.R_gt, s.t_gt)
        pose["Rt"][:, b] = MR.many(gt, K, 500 + b) if K > 2 else MR.perturbed(gt, K, 9 + b, 1e-2, 2e-2)
    if K >= 16:
        pose["status"][2, :] = SC_ENOHYP
        pose["Rt"][4, 1][5] = np.nan
    return pose


def _assert_batch(got, exp, what=""):
    (gr, gp, gc), (er, ep, ec) = got, exp
    for b in range(gr.shape[1]):
        print(what, "problem", b, "count", gc[b].tolist(), "expected", ec[b].tolist(), "parent", gp[:8, b].tolist(), ep[:8, b].tolist(),
              "counts", gr["count"][:8, b].tolist(), er["count"][:8, b].tolist())
        assert gc[b].tolist() == ec[b].tolist(), (what, b)
        assert np.array_equal(gp[:, b], ep[:, b]), (what, b)
        assert np.ascontiguousarray(gr[:, b]).tobytes() == np.ascontiguousarray(er[:, b]).tobytes(), (what, b)


@pytest.mark.parametrize("K,soa,rule", [(1, False, {}), (2, False, dict(num=1, den=1)), (2, True, dict(measure=1)),
                                        (16, False, dict(min_count=4)), (16, True, dict(measure=1, num=1, den=8, compact=True)),
                                        (64, False, dict(compact=True)), (64, False, dict(num=7, den=8, score_mode=2))])
def test_the_batch_equals_the_reference_and_the_frame_form(pkg, O, reg, K, soa, rule):
    rule = dict(rule)
    score_mode = rule.pop("score_mode", 0)
    scenes = _scenes(pkg)
    problems = [(s.src, s.tgt) for s in scenes]
    src, tgt, offset = _pack(scenes, soa)
    p = _params(pkg, soa, score_mode=score_mode)
    pose = _poses(pkg, scenes, K)
    kw = {k: v for k, v in rule.items() if k != "compact"}
    flags = pkg.SC_MERGE_COMPACT if rule.get("compact") else 0
    got = reg.merge_poses_batch(src, tgt, offset, p, pose, flags=flags, **kw)
    exp = MR.batch(O, problems, pose["Rt"], MR.TAU, pose["status"], score_mode, **rule)
    _assert_batch(got, exp, f"K={K} soa={soa} {rule}")
    if K >= 16:
        assert (got[1][2] == -1).all() and got[1][4, 1] == -1 and (got[1][5, 1:] == got[1][1, 1:]).all() and (got[1][5, 1:] != 5).all()
        assert (got[2][1:, 0] < got[2][1:, 1]).all()  # something was folded in every problem but the smallest
    if not soa:  # the device form, stride 64, outputs pre-filled with sentinel bytes: the same bytes; d_count NULL
        import torch
        pose64 = _poses(pkg, scenes, K, pkg.api.POLISH_BATCH_RESULT_DTYPE)
        B = len(scenes)
        d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
        d_pose = torch.from_numpy(pose64.view(np.uint8).reshape(-1).copy()).cuda()
        d_out = torch.full((K * B * REC,), 0xAB, dtype=torch.uint8, device="cuda")
        d_parent = torch.full((K * B,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
        d_count = torch.full((2 * B,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        mp = pkg.make_merge_params(flags=flags, **kw)
        reg.merge_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, mp, d_pose.data_ptr(), 64, K, d_out.data_ptr(),
                                     d_parent.data_ptr(), d_count.data_ptr())
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == got[0].tobytes() and d_parent.cpu().numpy().tobytes() == got[1].tobytes()
        assert d_count.cpu().numpy().view(np.uint32).tobytes() == got[2].tobytes()
        assert d_pose.cpu().numpy().tobytes() == pose64.tobytes()  # d_pose is read, never written
        d_out.fill_(0xAB); d_parent.fill_(0x2B2B2B2B)
        torch.cuda.synchronize()
        reg.merge_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, mp, d_pose.data_ptr(), 64, K, d_out.data_ptr(),
                                     d_parent.data_ptr(), 0)
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == got[0].tobytes() and d_parent.cpu().numpy().tobytes() == got[1].tobytes()
    # equality 4: the frame form on the same problem (the batch call above ended every frame, so each problem is registered first)
    if K in (2, 16, 64):
        framed = 0
        for b, s in enumerate(scenes):
            if reg.register(s.src, s.tgt, params=_params(pkg, score_mode=score_mode))["status"] != SC_OK:
                # SC_ENOHYP leaves no frame.  Only problem 0 — three correspondences, which may hold no triangle — may go that way
                assert b == 0, f"problem {b} (n = {len(s.src)}) left no frame"
                continue
            framed += 1
            rec, parent, _, count = reg.merge_poses_frame(np.ascontiguousarray(pose[:, b]), flags=flags | pkg.SC_MERGE_STATUS, **kw)
            assert np.array_equal(parent, got[1][:, b]) and count.tolist() == got[2][b].tolist(), b
            assert rec.tobytes() == np.ascontiguousarray(got[0][:, b]).tobytes(), b
        assert framed >= 3


def test_the_planes_of_the_instances_batch_and_their_copies_merge(pkg, O, reg):
    """sc_register_instances_batch_device's d_res, stride 80, planes past nfound SC_ENOHYP, with perturbed copies of the found
    motions appended as further planes: every copy folds into a found motion, no plane without a motion is kept"""
    import torch
    problems = IB.scenes(pkg)
    B, K = len(problems), 4
    src, tgt = np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems])
    offset = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.uint32)
    total = int(offset[-1])
    p = pkg.make_params(**IB.KW, max_triangles=MR.kw_of()["max_triangles"])
    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    d_res = torch.zeros(K * B * 80, dtype=torch.uint8, device="cuda")
    d_label = torch.zeros(total, dtype=torch.int32, device="cuda"); d_nfound = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    reg.register_instances_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, K, 3, d_res.data_ptr(), d_label.data_ptr(),
                                        d_nfound.data_ptr())
    torch.cuda.synchronize()
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE).reshape(K, B)
    nfound = d_nfound.cpu().numpy()
    pose = np.concatenate([res, res], axis=0)  # (2 K, B): the planes, then a neighbour of every plane
    for b in range(B):
        for k in range(K):
            if res[k, b]["status"] == SC_OK:
                pose["Rt"][K + k, b] = MR.perturbed(res[k, b]["Rt"], 1, 40 + 7 * b + k, 1e-3, 2e-3)[0]
    d_pose = torch.from_numpy(pose.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.full((2 * K * B * REC,), 0xAB, dtype=torch.uint8, device="cuda")
    d_parent = torch.full((2 * K * B,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
    d_count = torch.full((2 * B,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    reg.merge_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), offset, p, pkg.make_merge_params(), d_pose.data_ptr(), 80, 2 * K,
                                 d_out.data_ptr(), d_parent.data_ptr(), d_count.data_ptr())
    torch.cuda.synchronize()
    out = np.frombuffer(d_out.cpu().numpy().tobytes(), pkg.MERGE_POSE_DTYPE).reshape(2 * K, B)
    parent = d_parent.cpu().numpy().reshape(2 * K, B)
    count = d_count.cpu().numpy().view(np.uint32).reshape(B, 2)
    print("nfound", nfound.tolist(), "count", count.tolist(), "parent", parent.T.tolist())
    assert nfound.max() >= 2
    exp = MR.batch(O, problems, pose["Rt"], IB.KW["tau"], pose["status"])
    _assert_batch((out, parent, count), exp)
    for b in range(B):
        assert count[b].tolist()[1] == 2 * nfound[b] and count[b][0] <= nfound[b]  # a motion and its neighbour are one
        for k in range(2 * K):
            assert (parent[k, b] >= 0) == (k % K < nfound[b])  # a plane without a motion is out


def test_a_nan_coordinate_is_einval_alone_and_position_does_not_matter(pkg, O, reg):
    scenes = _scenes(pkg)
    K = 16
    pose = _poses(pkg, scenes, K)
    p = _params(pkg)
    src, tgt, offset = _pack(scenes)
    clean = reg.merge_poses_batch(src, tgt, offset, p, pose)
    bad_tgt = tgt.copy(); bad_tgt[int(offset[2]) + 7, 1] = np.nan  # problem 2, between two good ones
    rec, parent, count = reg.merge_poses_batch(src, bad_tgt, offset, p, pose)
    lo, hi = int(offset[2]), int(offset[3])
    assert (parent[:, 2] == -1).all() and (rec["status"][:, 2] == SC_EINVAL).all() and not rec["score"][:, 2].any() and not rec["count"][:, 2].any()
    assert count[2].tolist() == [0, 0] and (rec["index"][:, 2] == -1).all() and all(r.tobytes() == MR.IDENT.tobytes() for r in rec["Rt"][:, 2])
    for b in (0, 1, 3):
        assert np.ascontiguousarray(rec[:, b]).tobytes() == np.ascontiguousarray(clean[0][:, b]).tobytes() and count[b].tolist() == clean[2][b].tolist()
        assert np.array_equal(parent[:, b], clean[1][:, b])
    problems = [(s.src, s.tgt) for s in scenes]
    problems[2] = (scenes[2].src, bad_tgt[lo:hi])
    _assert_batch((rec, parent, count), MR.batch(O, problems, pose["Rt"], MR.TAU, pose["status"]), "a NaN in problem 2")
    # position independence: problem 3 first, last and alone, in batches of 6, 2 and 1 problems: the same bytes
    order = [3, 0, 1, 2, 1, 3]
    s6, t6, o6 = _pack([scenes[b] for b in order])
    r6, p6, c6 = reg.merge_poses_batch(s6, t6, o6, p, np.ascontiguousarray(pose[:, order]))
    for pos, b in enumerate(order):
        assert np.array_equal(p6[:, pos], clean[1][:, b]) and c6[pos].tolist() == clean[2][b].tolist(), pos
        assert np.ascontiguousarray(r6[:, pos]).tobytes() == np.ascontiguousarray(clean[0][:, b]).tobytes(), pos
    s1, t1, o1 = _pack([scenes[3]])
    r1, p1, c1 = reg.merge_poses_batch(s1, t1, o1, p, np.ascontiguousarray(pose[:, 3:4]))
    assert np.array_equal(p1[:, 0], clean[1][:, 3]) and r1.tobytes() == np.ascontiguousarray(clean[0][:, 3:4]).tobytes() and c1[0].tolist() == clean[2][3].tolist()


def test_refusals_and_the_entry_ends_the_frame(pkg, O):
    scenes = _scenes(pkg)
    src, tgt, offset = _pack(scenes)
    r = pkg.Registrar(0)
    try:
        p = _params(pkg)
        pose = _poses(pkg, scenes, 2)
        for what, kw, word in (("measure 2", dict(measure=2), "measure"), ("num 0", dict(num=0), "num"), ("num above den", dict(num=5, den=4), "num"),
                               ("den 65537", dict(den=65537), "den"), ("a mask", dict(sel_mode=1), "sel_mode"), ("flag 4", dict(flags=4), "flag")):
            with pytest.raises(pkg.SacCotError) as e:
                r.merge_poses_batch(src, tgt, offset, p, pose, **kw)
            print(what, e.value)
            assert e.value.status == SC_EINVAL and word in str(e.value) and "sc_merge_poses_batch" in str(e.value), what
        with pytest.raises(pkg.SacCotError) as e:
            r.merge_poses_batch(src, tgt, offset, p, _poses(pkg, scenes, 65))
        assert e.value.status == SC_EINVAL and "n_poses" in str(e.value)
        with pytest.raises(pkg.SacCotError) as e:
            r.merge_poses_batch(src, tgt, np.array([0, 2], np.uint32), p, pose[:, :1])  # a problem of two correspondences
        assert e.value.status == SC_EINVAL
        s = scenes[3]
        assert r.register(s.src, s.tgt, params=p)["status"] == SC_OK
        r.merge_poses_batch(src, tgt, offset, p, pose)
        r._frame_n = len(s.src)
        with pytest.raises(pkg.SacCotError) as e:
            r.merge_poses_frame(pose["Rt"][:, 3])
        assert e.value.status == SC_EINVAL and "no frame" in str(e.value)
        # a call outstanding on the context: refused until sc_wait, then the same bytes as before
        import torch
        before = r.merge_poses_batch(src, tgt, offset, p, pose)
        n = len(s.src)
        ds, dt = torch.from_numpy(s.src).cuda(), torch.from_numpy(s.tgt).cuda()
        d_Rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
        r.register_device_async(ds.data_ptr(), dt.data_ptr(), n, p, d_Rt.data_ptr(), d_mask.data_ptr())
        with pytest.raises(pkg.SacCotError) as e:
            r.merge_poses_batch(src, tgt, offset, p, pose)
        assert e.value.status == SC_EINVAL and "outstanding" in str(e.value)
        assert r.wait()[0] == SC_OK
        after = r.merge_poses_batch(src, tgt, offset, p, pose)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after, before))
    finally:
        r.close()
