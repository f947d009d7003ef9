"""GPU: the fp64 information matrix of a batch's poses (include/saccot.h, sc_pose_info_batch / _device / _slots_device and
sc_pose_info_pairs_slots_device).

The expected value of every case is tests/pose_info_ref.py — Python loops over numpy float64 scalars in the contract's order, the
inlier set from the CPU restatement's mask — and every comparison is bit for bit: the 320 bytes of every record (`tobytes`).  No
tolerances.  The scenes are checked on the CPU by tests/test_pose_info_abi.py.
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref
import match_batch_ref as M
import pose_info_ref as PI

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
REC = 320


def _pack(problems):
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.uint32)
    return np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems]), off


def _layout(src, tgt, soa):
    return (np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)) if soa else (src, tgt)


def _params(pkg, tau, soa=False, **kw):
    return pkg.make_params(**PI.kw_of(tau), layout=pkg.SC_SOA if soa else pkg.SC_AOS, **kw)


def _records(pkg, t):
    return np.frombuffer(t.cpu().numpy().tobytes(), pkg.POSE_INFO_RESULT_DTYPE)


def _junk_info(torch, nb):
    return torch.full((nb * REC,), 0xAB, dtype=torch.uint8, device="cuda")


def _assert_info(got, exp, what=""):
    assert len(got) == len(exp), what
    for b in range(len(got)):
        print(what, b, int(got[b]["status"]), int(got[b]["inliers"]), float(got[b]["sse"]), "| expected", int(exp[b]["status"]),
              int(exp[b]["inliers"]), float(exp[b]["sse"]))
        assert got[b].tobytes() == exp[b].tobytes(), (what, b)


def _zero(status):
    z = np.zeros((), PI.RESULT_DTYPE); z["status"] = status
    return z.tobytes()


# ---- 1: the packed form: poses from sc_register_batch (stride 80) and sc_polish_batch (stride 64), hand-made ones for the crafted scenes
@pytest.mark.parametrize("tau", PI.TAUS)
def test_mixed_batch_behind_register_and_polish_equals_the_reference(pkg, O, reg, tau):
    import torch
    problems = PI.mixed(pkg)
    nb = len(problems)
    q = pkg.make_polish_params(candidates=1, max_iter=16)
    seen = None
    for soa in (False, True):
        src, tgt, off = _pack(problems)
        src, tgt = _layout(src, tgt, soa)
        p = _params(pkg, tau, soa)
        d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
        d_res = torch.zeros(nb * 80, dtype=torch.uint8, device="cuda"); d_pol = torch.zeros(nb * 64, dtype=torch.uint8, device="cuda")
        d_mask = torch.zeros(int(off[-1]), dtype=torch.uint8, device="cuda")
        d_i80, d_i64 = _junk_info(torch, nb), _junk_info(torch, nb)
        torch.cuda.synchronize()
        # one context, four launches, no host word in between
        reg.register_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_res.data_ptr(), d_mask.data_ptr())
        reg.polish_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, q, d_res.data_ptr(), d_pol.data_ptr(), d_mask.data_ptr())
        reg.pose_info_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_res.data_ptr(), 80, d_i80.data_ptr())
        reg.pose_info_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_pol.data_ptr(), 64, d_i64.data_ptr())
        torch.cuda.synchronize()
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE)
        pol = np.frombuffer(d_pol.cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE)
        i80, i64 = _records(pkg, d_i80), _records(pkg, d_i64)
        assert (res["status"] == SC_OK).sum() >= 9 and list(pol["status"]) == list(res["status"])
        _assert_info(i80, PI.batch(O, problems, res, tau), f"tau={tau} soa={soa} stride 80")
        _assert_info(i64, PI.batch(O, problems, pol, tau), f"tau={tau} soa={soa} stride 64")
        ok = res["status"] == SC_OK
        assert np.array_equal(i80["inliers"][ok], res["best_count"][ok])  # the inlier test is the masks'
        assert np.array_equal(i64["inliers"][ok], pol["score"][ok]) and int(i64["inliers"][-1]) >= 3  # (n = 512: eight chunks)
        for b in np.flatnonzero(~ok):
            assert i80[b].tobytes() == i64[b].tobytes() == _zero(res["status"][b])
        # the host form == the device form
        assert reg.pose_info_batch_raw(src, tgt, off, p, res).tobytes() == i80.tobytes()
        assert reg.pose_info_batch_raw(src, tgt, off, p, pol).tobytes() == i64.tobytes()
        if seen is None:
            seen = (i80.tobytes(), i64.tobytes())
        else:  # the layout of the points does not matter
            assert (i80.tobytes(), i64.tobytes()) == seen


@pytest.mark.parametrize("tau", PI.TAUS)
def test_crafted_scenes_equal_the_reference(pkg, O, reg, tau):
    import torch
    names, problems, poses = PI.crafted()
    exp = PI.batch(O, problems, poses, tau)
    assert [int(e["inliers"]) for e in exp][:1] + [int(e["inliers"]) for e in exp][2:] == [1, 0, 2, 70]
    for soa in (False, True):
        src, tgt, off = _pack(problems)
        src, tgt = _layout(src, tgt, soa)
        p = _params(pkg, tau, soa)
        got = reg.pose_info_batch_raw(src, tgt, off, p, poses)
        _assert_info(got, exp, f"crafted {names} tau={tau} soa={soa}")
        d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
        d_pose = torch.from_numpy(np.frombuffer(poses.tobytes(), np.uint8).copy()).cuda()
        d_info = _junk_info(torch, len(problems))
        torch.cuda.synchronize()
        reg.pose_info_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_pose.data_ptr(), 80, d_info.data_ptr())
        torch.cuda.synchronize()
        assert _records(pkg, d_info).tobytes() == got.tobytes()
        assert d_pose.cpu().numpy().tobytes() == poses.tobytes()  # d_pose is read, never written
    # a pose record of the smallest stride: 52 bytes
    small = np.zeros(len(problems), np.dtype([("Rt", np.float32, 12), ("status", np.int32)]))
    small["Rt"], small["status"] = poses["Rt"], poses["status"]
    src, tgt, off = _pack(problems)
    assert reg.pose_info_batch_raw(src, tgt, off, _params(pkg, tau), small).tobytes() == exp.tobytes()


# ---- 2: statuses: each affects only its own problem ----------------------------------------------------------------------------------
def test_bad_problems_between_good_ones(pkg, O, reg):
    tau = 0.02
    g128, g64, g65, g129, g63 = (batch_ref.scene(pkg, n, .3) for n in (128, 64, 65, 129, 63))
    clean = [g128, g64, g63, g129, g65]
    src, tgt, off = _pack(clean)
    p = _params(pkg, tau)
    recs, _ = reg.register_batch_raw(src, tgt, off, p)
    assert [int(recs["status"][k]) for k in (0, 1, 3, 4)] == [SC_OK] * 4
    nan_t = g64[1].copy(); nan_t[17, 2] = np.nan
    problems = [g128, (g64[0], nan_t), g63, g129, g65]  # [1]: a NaN coordinate under an SC_OK record
    hand = recs.copy()
    hand["status"][2] = SC_ENOHYP                       # [2]: a passed-through SC_ENOHYP
    hand["Rt"][3][5] = np.nan                           # [3]: an SC_OK record with a NaN in Rt
    src, tgt, _ = _pack(problems)
    for soa in (False, True):
        a, b = _layout(src, tgt, soa)
        got = reg.pose_info_batch_raw(a, b, off, _params(pkg, tau, soa), hand)
        _assert_info(got, PI.batch(O, problems, hand, tau), f"soa={soa}")
        assert list(got["status"]) == [SC_OK, SC_EINVAL, SC_ENOHYP, SC_EINVAL, SC_OK]
        for k, st in ((1, SC_EINVAL), (2, SC_ENOHYP), (3, SC_EINVAL)):
            assert got[k].tobytes() == _zero(st)
        # the neighbours are bit-identical to a batch without the bad ones
        fs, ft, foff = _pack([g128, g65])
        fa, fb = _layout(fs, ft, soa)
        few = reg.pose_info_batch_raw(fa, fb, foff, _params(pkg, tau, soa), hand[[0, 4]])
        assert few[0].tobytes() == got[0].tobytes() and few[1].tobytes() == got[4].tobytes() and int(few["inliers"].min()) >= 3


# ---- 3: a record is a function of its own problem, its pose and tau -------------------------------------------------------------------
def test_independence_of_position_neighbours_and_batch_size(pkg, O, reg):
    tau = 0.02
    problems = PI.mixed(pkg)
    src, tgt, off = _pack(problems)
    p = _params(pkg, tau)
    recs, _ = reg.register_batch_raw(src, tgt, off, p)
    base = reg.pose_info_batch_raw(src, tgt, off, p, recs)
    _assert_info(base, PI.batch(O, problems, recs, tau), "base")

    def check(order, what):
        s, t, o = _pack([problems[b] for b in order])
        got = reg.pose_info_batch_raw(s, t, o, p, recs[list(order)])
        for pos, b in enumerate(order):
            assert got[pos].tobytes() == base[b].tobytes(), (what, b)

    nb = len(problems)
    check(list(range(nb))[::-1], "reversed")
    for b in range(nb):
        check([b], "alone")


# ---- 4: more workgroups than the device holds at once --------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [1100, 2600])
def test_many_copies_of_three_small_problems(pkg, O, reg, copies):
    _, problems, poses = PI.crafted()
    pick = [2, 3, 0]  # none (n = 64), two (n = 65), last (n = 129)
    three = [problems[k] for k in pick]
    exp = PI.batch(O, three, poses[pick], 0.05)
    src, tgt, off = _pack([three[b % 3] for b in range(copies)])
    got = reg.pose_info_batch_raw(src, tgt, off, _params(pkg, 0.05), poses[[pick[b % 3] for b in range(copies)]])
    assert len(got) == copies
    for k in range(3):
        assert {r.tobytes() for r in got[k::3]} == {exp[k].tobytes()}, k


# ---- 5: the slot form behind sc_register_batch_features_device -----------------------------------------------------------------------
def _slots_expected(O, problems, so, knn, corr, count, poses, tau):
    exp = np.zeros(len(problems), PI.RESULT_DTYPE)
    for b, s in enumerate(problems):
        lo, cap = int(so[b]) * knn, len(s[0]) * knn
        exp[b] = PI.slots_one(O, s[0], s[2], corr[lo: lo + cap], int(count[b, 0]), int(count[b, 1]), poses[b]["status"], poses[b]["Rt"], tau)
    return exp


@pytest.mark.parametrize("mode", ["mutual", "knn2"])
def test_slot_form_behind_the_features_entry(pkg, O, reg, mode):
    import torch
    tau = 0.02
    knn = 1 if mode == "mutual" else 2
    scenes = [M.feature_scene(n, rho, noise, 4100 + n) for n, rho, noise in ((40, .6, .001), (1, 1.0, 0.0), (100, .4, .001), (64, .5, .001), (200, .3, .001))]
    problems = [list(s[:4]) for s in scenes]
    problems[3][1] = problems[3][1].copy(); problems[3][1][5, 0] = np.inf  # a non-finite descriptor: the match flags this problem
    mp = pkg.api.make_match_params(33, knn=knn, mutual=(mode == "mutual"))
    so = reg._offsets([len(s[1]) for s in problems]); to = reg._offsets([len(s[3]) for s in problems])
    fsrc, ftgt = np.concatenate([s[1] for s in problems]), np.concatenate([s[3] for s in problems])
    nb, slots = len(problems), int(so[-1]) * knn
    q = pkg.make_polish_params(candidates=1, max_iter=16)
    kw = dict(M.KW, tau=tau)
    seen = None
    for soa in (False, True):
        p = pkg.make_params(**kw, layout=pkg.SC_SOA if soa else pkg.SC_AOS)
        src, tgt = _layout(np.concatenate([s[0] for s in problems]), np.concatenate([s[2] for s in problems]), soa)
        dev = {k: torch.from_numpy(v).cuda() for k, v in dict(src=src, fsrc=fsrc, tgt=tgt, ftgt=ftgt).items()}
        d_res = torch.zeros(nb * 80, dtype=torch.uint8, device="cuda"); d_pol = torch.zeros(nb * 64, dtype=torch.uint8, device="cuda")
        d_corr = torch.full((slots, 2), -7, dtype=torch.int32, device="cuda"); d_d2 = torch.zeros(slots, dtype=torch.float32, device="cuda")
        d_count = torch.full((nb, 2), 9, dtype=torch.int32, device="cuda")
        d_mask = torch.zeros(slots, dtype=torch.uint8, device="cuda")
        d_i80, d_i64 = _junk_info(torch, nb), _junk_info(torch, nb)
        torch.cuda.synchronize()
        reg.register_batch_features_device(dev["src"].data_ptr(), dev["fsrc"].data_ptr(), so, dev["tgt"].data_ptr(), dev["ftgt"].data_ptr(), to,
                                           mp, p, d_res.data_ptr(), d_corr.data_ptr(), d_d2.data_ptr(), d_count.data_ptr(), d_mask.data_ptr())
        reg.polish_batch_slots_device(dev["src"].data_ptr(), so, dev["tgt"].data_ptr(), to, knn, p, q, d_corr.data_ptr(), d_count.data_ptr(),
                                      d_res.data_ptr(), d_pol.data_ptr(), d_mask.data_ptr())
        reg.pose_info_batch_slots_device(dev["src"].data_ptr(), so, dev["tgt"].data_ptr(), to, knn, p, d_corr.data_ptr(), d_count.data_ptr(),
                                         d_res.data_ptr(), 80, d_i80.data_ptr())
        reg.pose_info_batch_slots_device(dev["src"].data_ptr(), so, dev["tgt"].data_ptr(), to, knn, p, d_corr.data_ptr(), d_count.data_ptr(),
                                         d_pol.data_ptr(), 64, d_i64.data_ptr())
        torch.cuda.synchronize()
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE)
        pol = np.frombuffer(d_pol.cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE)
        corr, count = d_corr.cpu().numpy(), d_count.cpu().numpy().astype(np.uint32)
        i80, i64 = _records(pkg, d_i80), _records(pkg, d_i64)
        print(mode, soa, list(res["status"]), count.tolist())
        assert list(res["status"]) == [SC_OK, SC_ENOHYP, SC_OK, SC_EINVAL, SC_OK] and count[1, 0] < 3 and count[3].tolist() == [0, 1]
        _assert_info(i80, _slots_expected(O, problems, so, knn, corr, count, res, tau), f"slots {mode} soa={soa} stride 80")
        _assert_info(i64, _slots_expected(O, problems, so, knn, corr, count, pol, tau), f"slots {mode} soa={soa} stride 64")
        # the short and the flagged problem pass their input status through; the others hold a matrix
        assert i80[1].tobytes() == _zero(SC_ENOHYP) and i80[3].tobytes() == _zero(SC_EINVAL)
        assert all(int(i64[b]["status"]) == SC_OK and int(i64[b]["inliers"]) >= 3 for b in (0, 2, 4))
        # ... and a record that claims SC_OK for them does not make them fit
        claim = res.copy(); claim["status"][[1, 3]] = SC_OK
        d_claim = torch.from_numpy(np.frombuffer(claim.tobytes(), np.uint8).copy()).cuda()
        # one corrupted index in problem 2's slot: an index outside the problem
        bad_corr = corr.copy(); bad_corr[int(so[2]) * knn + 1, 1] = len(problems[2][2])
        d_bad = torch.from_numpy(bad_corr).cuda()
        d_i2 = _junk_info(torch, nb)
        torch.cuda.synchronize()
        reg.pose_info_batch_slots_device(dev["src"].data_ptr(), so, dev["tgt"].data_ptr(), to, knn, p, d_bad.data_ptr(), d_count.data_ptr(),
                                         d_claim.data_ptr(), 80, d_i2.data_ptr())
        torch.cuda.synchronize()
        i2 = _records(pkg, d_i2)
        _assert_info(i2, _slots_expected(O, problems, so, knn, bad_corr, count, claim, tau), f"slots {mode} soa={soa} corrupted")
        assert [i2[b].tobytes() for b in (1, 2, 3)] == [_zero(SC_EINVAL)] * 3
        assert i2[0].tobytes() == i80[0].tobytes() and i2[4].tobytes() == i80[4].tobytes()  # only their own problems
        if seen is None:
            seen = (i80.tobytes(), i64.tobytes())
        else:  # the layout of the points does not matter
            assert (i80.tobytes(), i64.tobytes()) == seen


# ---- 6: the pairs form equals the slot form on the expanded arrays -----------------------------------------------------------------------
def test_pairs_form_equals_the_slot_form_on_the_expanded_list(pkg, O, reg):
    import torch
    tau, knn = 0.02, 1
    scenes = [M.feature_scene(n, rho, noise, 4200 + n) for n, rho, noise in ((64, .5, .001), (100, .4, .001), (40, .6, .001))]
    sets = []
    for s in scenes:
        sets += [(s[0], s[1]), (s[2], s[3])]  # six sets: the two sides of three scenes
    set_off = np.concatenate([[0], np.cumsum([len(a) for a, _ in sets])]).astype(np.uint32)
    pairs = np.array([(2, 3), (0, 1), (4, 5), (0, 3), (2, 3), (1, 1), (5, 4)], np.uint32)  # (2, 3) twice; (1, 1): a set with itself
    mp = pkg.api.make_match_params(33, knn=knn, mutual=True)
    p = pkg.make_params(**dict(M.KW, tau=tau))
    q = pkg.make_polish_params(candidates=1, max_iter=16)
    npairs = len(pairs)

    def outputs(slots):
        return dict(res=torch.zeros(npairs * 80, dtype=torch.uint8, device="cuda"), pol=torch.zeros(npairs * 64, dtype=torch.uint8, device="cuda"),
                    corr=torch.full((slots, 2), -7, dtype=torch.int32, device="cuda"), d2=torch.zeros(slots, dtype=torch.float32, device="cuda"),
                    count=torch.full((npairs, 2), 9, dtype=torch.int32, device="cuda"), mask=torch.zeros(slots, dtype=torch.uint8, device="cuda"),
                    info=_junk_info(torch, npairs))

    # the table and the list
    slot = reg.pairs_layout(set_off, pairs, knn)
    d_pts = torch.from_numpy(np.concatenate([a for a, _ in sets])).cuda()
    d_feat = torch.from_numpy(np.concatenate([f for _, f in sets])).cuda()
    o = outputs(int(slot[-1]))
    torch.cuda.synchronize()
    reg.register_pairs_features_device(d_pts.data_ptr(), d_feat.data_ptr(), set_off, pairs, mp, p, o["res"].data_ptr(), o["corr"].data_ptr(),
                                       o["d2"].data_ptr(), o["count"].data_ptr(), o["mask"].data_ptr())
    reg.polish_pairs_slots_device(d_pts.data_ptr(), set_off, pairs, knn, p, q, o["corr"].data_ptr(), o["count"].data_ptr(), o["res"].data_ptr(),
                                  o["pol"].data_ptr(), o["mask"].data_ptr())
    reg.pose_info_pairs_slots_device(d_pts.data_ptr(), set_off, pairs, knn, p, o["corr"].data_ptr(), o["count"].data_ptr(), o["pol"].data_ptr(), 64,
                                     o["info"].data_ptr())
    torch.cuda.synchronize()
    got = _records(pkg, o["info"])
    pol = np.frombuffer(o["pol"].cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE)
    corr, count = o["corr"].cpu().numpy(), o["count"].cpu().numpy().astype(np.uint32)

    # the list expanded into packed arrays in list order, and the slot form on them
    problems = [(sets[a][0], sets[a][1], sets[b][0], sets[b][1]) for a, b in pairs.tolist()]
    so = reg._offsets([len(s[0]) for s in problems]); to = reg._offsets([len(s[2]) for s in problems])
    assert np.array_equal(so.astype(np.int64) * knn, slot.astype(np.int64))
    d_ps = torch.from_numpy(np.concatenate([s[0] for s in problems])).cuda(); d_fs = torch.from_numpy(np.concatenate([s[1] for s in problems])).cuda()
    d_pt = torch.from_numpy(np.concatenate([s[2] for s in problems])).cuda(); d_ft = torch.from_numpy(np.concatenate([s[3] for s in problems])).cuda()
    e = outputs(int(so[-1]) * knn)
    torch.cuda.synchronize()
    reg.register_batch_features_device(d_ps.data_ptr(), d_fs.data_ptr(), so, d_pt.data_ptr(), d_ft.data_ptr(), to, mp, p, e["res"].data_ptr(),
                                       e["corr"].data_ptr(), e["d2"].data_ptr(), e["count"].data_ptr(), e["mask"].data_ptr())
    reg.polish_batch_slots_device(d_ps.data_ptr(), so, d_pt.data_ptr(), to, knn, p, q, e["corr"].data_ptr(), e["count"].data_ptr(), e["res"].data_ptr(),
                                  e["pol"].data_ptr(), e["mask"].data_ptr())
    reg.pose_info_batch_slots_device(d_ps.data_ptr(), so, d_pt.data_ptr(), to, knn, p, e["corr"].data_ptr(), e["count"].data_ptr(),
                                     e["pol"].data_ptr(), 64, e["info"].data_ptr())
    torch.cuda.synchronize()
    exp = _records(pkg, e["info"])
    assert e["pol"].cpu().numpy().tobytes() == pol.tobytes()
    _assert_info(got, exp, "pairs vs slots")
    _assert_info(got, _slots_expected(O, problems, so, knn, corr, count, pol, tau), "pairs vs the reference")
    assert got[0].tobytes() == got[4].tobytes()  # the repeated pair
    assert sum(int(r["status"]) == SC_OK and int(r["inliers"]) >= 3 for r in got) >= 4
    assert int(got[5]["status"]) == int(pol[5]["status"])  # the pair of a set with itself: whatever its registration said


# ---- 7: what is refused, and what a call leaves -------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(pkg, O, reg):
    L = reg._lib
    tau = 0.02
    s, t = batch_ref.scene(pkg, 128, .3)
    off = np.array([0, 128], np.uint32)
    p = _params(pkg, tau)
    recs, _ = reg.register_batch_raw(s, t, off, p)
    good = reg.pose_info_batch_raw(s, t, off, p, recs)
    assert good[0]["status"] == SC_OK and good.tobytes() == PI.batch(O, [(s, t)], recs, tau).tobytes()
    u32 = lambda *a: np.array(a, np.uint32)  # noqa: E731
    three = np.zeros(3, pkg.BATCH_RESULT_DTYPE)

    def host(o, nb, pp, stride, pose=recs):
        info = np.zeros(max(nb, 1), PI.RESULT_DTYPE)
        rc = L.sc_pose_info_batch(reg._h, s.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_float)),
                                  o.ctypes.data_as(C.POINTER(C.c_uint32)), nb, C.byref(pp), pose.ctypes.data_as(C.c_void_p), stride,
                                  info.ctypes.data_as(C.c_void_p))
        return rc, L.sc_last_error(reg._h).decode()

    cases = {
        "stride 0": lambda: host(off, 1, p, 0),
        "stride 50": lambda: host(off, 1, p, 50),
        "stride 54": lambda: host(off, 1, p, 54),
        "n_b = 2": lambda: host(u32(0, 2), 1, p, 80),
        "a decreasing offset": lambda: host(u32(0, 64, 60, 128), 3, p, 80, three),
        "shard_world = 2": lambda: host(off, 1, _params(pkg, tau, shard_world=2), 80),
    }
    for what, call in cases.items():
        rc, err = call()
        print(what, rc, err)
        assert rc == SC_EINVAL and err and "sc_pose_info_batch" in err, what
        assert reg.pose_info_batch_raw(s, t, off, p, recs).tobytes() == good.tobytes(), what  # the context stays usable
    # a call ends the frame and leaves none
    assert reg.register(s, t, params=p)["status"] == SC_OK
    reg.pose_info_batch_raw(s, t, off, p, recs)
    for call in (reg.peel, reg.polish):
        with pytest.raises(pkg.SacCotError) as e:
            call()
        assert e.value.status == SC_EINVAL


# ---- 8: a context that never calls these entries allocates nothing new ----------------------------------------------------------------
def test_workspace_appears_with_the_first_call(pkg):
    r = pkg.Registrar(0)
    try:
        s, t = batch_ref.scene(pkg, 128, .3)
        off = np.array([0, 128], np.uint32)
        p = _params(pkg, 0.02)
        recs, _ = r.register_batch_raw(s, t, off, p)
        first = r.register(s, t, params=p)["stats"]["workspace_bytes"]
        assert r.register(s, t, params=p)["stats"]["workspace_bytes"] == first
        r.pose_info_batch_raw(s, t, off, p, recs)
        second = r.register(s, t, params=p)["stats"]["workspace_bytes"]
        r.pose_info_batch_raw(s, t, off, p, recs)
        print(first, second)
        assert second > first and r.register(s, t, params=p)["stats"]["workspace_bytes"] == second
    finally:
        r.close()
