"""GPU: Gauss-Newton pose-graph solve of a pair list's sets (include/saccot.h, sc_pairs_solve / sc_pairs_solve_device).

The expected value of every case is tests/solve_ref.py — numpy fp64 in the header's order, the 64 slots, the fold and the grand sums
restated literally, fed the three thresholds the library itself derives (sc_solve_thresholds) — and every comparison is bit for bit:
the 160 bytes of every set's record, the 48 of every pair's and the 64 of the summary, doubles compared as their bytes.  No
tolerances.  Two cases hold the library to something other than that reference: the sets exact in integers (an np.int64 expectation,
below) and, through the reference, the dense solver of tests/test_solve_abi.py.
"""
import ctypes as C

import numpy as np
import pytest

import cycles_ref as CR
import match_batch_ref as M
import merge_ref as MR
import solve_ref as V
import sync_ref as SR

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
SET, PAIR, SUM, INIT = 160, 48, 64, 160


def _params(pkg, f, **kw):
    p = dict(f.params); p.update(kw)
    return pkg.make_solve_params(**p)


def _expected(pkg, f, vp, init):
    thr = pkg.solve_thresholds(vp)
    return V.solve(f.n_sets, f.pairs, f.rt, init[0], init[1], thr[0], thr[1], thr[2], anchor=vp.anchor, max_outer=vp.max_outer, max_inner=vp.max_inner,
                   use=f.use, info=f.info, info_statuses=f.info_statuses if vp.flags & V.INFO_STATUS else None,
                   statuses=f.statuses if vp.flags & V.STATUS else None)


def _assert_same(got, exp, what=""):
    (gs, gp, gm), (es, ep, em) = got, exp
    print(what, "summary", gm, "expected", em, "set records that differ",
          int((gs.view(np.uint8).reshape(-1, SET) != es.view(np.uint8).reshape(-1, SET)).any(axis=1).sum()), "pair records that differ",
          int((gp.view(np.uint8).reshape(-1, PAIR) != ep.view(np.uint8).reshape(-1, PAIR)).any(axis=1).sum()))
    assert np.asarray(gm).tobytes() == np.asarray(em).tobytes(), what
    for name in es.dtype.names:
        assert gs[name].tobytes() == es[name].tobytes(), (what, "set", name)
    for name in ep.dtype.names:
        assert gp[name].tobytes() == ep[name].tobytes(), (what, "pair", name)
    assert gs.tobytes() == es.tobytes() and gp.tobytes() == ep.tobytes(), what


def _records(rt, stride, statuses=None):
    """the poses as records of `stride` bytes: Rt at byte 0, the status at byte 48 where there is room, 0xA5 elsewhere"""
    raw = np.full((len(rt), stride), 0xA5, np.uint8)
    raw[:, :48] = np.ascontiguousarray(rt, np.float32).view(np.uint8).reshape(len(rt), 48)
    if stride >= 52:
        st = np.zeros(len(rt), np.int32) if statuses is None else np.asarray(statuses, np.int32)
        raw[:, 48:52] = st.view(np.uint8).reshape(len(rt), 4)
    return raw


def _info_records(info, stride, statuses=None):
    """the matrices as records of `stride` bytes: 36 doubles at byte 0, the status at byte 296 where there is room, 0xA5 elsewhere"""
    raw = np.full((len(info), stride), 0xA5, np.uint8)
    raw[:, :288] = np.ascontiguousarray(info, np.float64).view(np.uint8).reshape(len(info), 288)
    if stride >= 300:
        st = np.zeros(len(info), np.int32) if statuses is None else np.asarray(statuses, np.int32)
        raw[:, 296:300] = st.view(np.uint8).reshape(len(info), 4)
    return raw


def _init_records(X, status, stride=INIT):
    raw = np.full((len(X), stride), 0xA5, np.uint8)
    raw[:, 48:52] = np.ascontiguousarray(status, np.int32).view(np.uint8).reshape(len(X), 4)
    raw[:, 64:160] = np.ascontiguousarray(X, np.float64).view(np.uint8).reshape(len(X), 96)
    return raw


def _fetch(pkg, d_set, d_pair, d_sum):
    return (np.frombuffer(d_set.cpu().numpy().tobytes(), pkg.SOLVE_SET_DTYPE), np.frombuffer(d_pair.cpu().numpy().tobytes(), pkg.SOLVE_PAIR_DTYPE),
            np.frombuffer(d_sum.cpu().numpy().tobytes(), pkg.SOLVE_SUMMARY_DTYPE)[0])


def _outputs(n_sets, P):
    import torch
    return (torch.full((n_sets * SET,), 0xAB, dtype=torch.uint8, device="cuda"), torch.full((P * PAIR,), 0xAC, dtype=torch.uint8, device="cuda"),
            torch.full((SUM,), 0xCD, dtype=torch.uint8, device="cuda"))


def _device(pkg, r, f, vp, init, pose_stride=None, info_stride=None, use_stride=4, init_stride=INIT, identity_records=False):
    """the device form on host data: copies in, one call, one device-wide wait -> (sets, pairs, summary); the outputs are pre-filled
    with sentinel bytes"""
    import torch
    P = len(f.pairs)
    pose_stride = pose_stride or (64 if vp.flags & V.STATUS else 48)
    raw = _records(f.rt, pose_stride, f.statuses)
    d_pose = torch.from_numpy(raw.reshape(-1).copy()).cuda()
    d_use = None
    if f.use is not None:
        words = np.full((P, use_stride), 0xA5, np.uint8)
        words[:, :4] = np.ascontiguousarray(f.use, np.uint32).view(np.uint8).reshape(P, 4)
        d_use = torch.from_numpy(words.reshape(-1)).cuda()
    d_info, info = None, f.info
    if info is None and identity_records:
        info = np.tile(np.eye(6).ravel(), (P, 1))
    if info is not None:
        info_stride = info_stride or (320 if vp.flags & V.INFO_STATUS else 288)
        iraw = _info_records(info, info_stride, f.info_statuses)
        d_info = torch.from_numpy(iraw.reshape(-1).copy()).cuda()
    init_raw = _init_records(init[0], init[1], init_stride)
    d_init = torch.from_numpy(init_raw.reshape(-1).copy()).cuda()
    d_set, d_pair, d_sum = _outputs(f.n_sets, P)
    torch.cuda.synchronize()
    r.pairs_solve_device(f.n_sets, f.pairs, vp, d_pose.data_ptr(), pose_stride, 0 if d_use is None else d_use.data_ptr(), use_stride,
                         0 if d_info is None else d_info.data_ptr(), info_stride or 288, d_init.data_ptr(), init_stride, d_set.data_ptr(),
                         d_pair.data_ptr(), d_sum.data_ptr())
    torch.cuda.synchronize()
    assert d_pose.cpu().numpy().tobytes() == raw.tobytes() and d_init.cpu().numpy().tobytes() == init_raw.tobytes()  # read, never written
    return _fetch(pkg, d_set, d_pair, d_sum)


def _host(pkg, r, f, vp, init):
    rec = np.frombuffer(_init_records(init[0], init[1]).tobytes(), pkg.SYNC_SET_DTYPE)
    pose = f.rt
    if vp.flags & V.STATUS:
        dt = np.dtype({"names": ["Rt", "status"], "formats": [("<f4", (12,)), "<i4"], "offsets": [0, 48], "itemsize": 64})
        pose = np.frombuffer(_records(f.rt, 64, f.statuses).tobytes(), dt)
    info = f.info
    if info is not None and vp.flags & V.INFO_STATUS:
        info = np.frombuffer(_info_records(f.info, 320, f.info_statuses).tobytes(), V.INFO_DTYPE)
    return r.pairs_solve(f.n_sets, f.pairs, pose, rec, vp, use=f.use, info=info)


def _both(pkg, reg, f, what, init=None, **kw):
    """the device form and the reference on a family, compared -> (got, expected)"""
    vp = _params(pkg, f, **kw)
    init = init or V.sync_start(f)
    exp = _expected(pkg, f, vp, init)
    got = _device(pkg, reg, f, vp, init)
    _assert_same(got, exp, what)
    return got, exp


# 1. sets exact in integers: the expectation is np.int64 and shares no code with the reference
@pytest.mark.parametrize("anchor", [0, 11])
def test_sets_exact_in_integers(pkg, reg, anchor):
    f = V.exact24(anchor)
    truth = SR.integers(SR.exact24(anchor), anchor)  # np.int64
    vp = _params(pkg, f)
    got = _device(pkg, reg, f, vp, (f.init_X, f.init_status))
    sets, res, s = got
    assert np.array_equal(sets["X"], truth) and np.array_equal(sets["Rt"], truth)  # nothing moved
    assert sets["X"].tobytes() == f.init_X.tobytes()  # ... bit for bit
    assert (int(s["outer"]), int(s["stop"]), int(s["inner_total"]), int(s["free_sets"]), int(s["used_pairs"])) == (1, pkg.SC_SOLVE_STOP_CONVERGED, 0, 23, 276)
    assert float(s["cost0"]) == 0.0 and float(s["cost"]) == 0.0 and float(s["rz0"]) == 0.0
    assert not res["cost"].any() and not res["w2"].any() and not res["v2"].any() and res["used"].all()
    assert sets["state"].tolist() == [pkg.SC_SOLVE_ANCHOR if k == anchor else pkg.SC_SOLVE_FREE for k in range(24)]
    _assert_same(got, _expected(pkg, f, vp, (f.init_X, f.init_status)), "exact24")


# 2. the ring of 40 and 24 sets with all pairs, noisy: behind sc_pairs_sync_device on one stream with no wait, and the host form
@pytest.mark.parametrize("name", ["ring40", "k24"])
def test_sync_then_solve_on_one_stream(pkg, reg, name):
    import torch
    f = getattr(V, name)()
    P = len(f.pairs)
    sp = pkg.make_sync_params(1e-4, 1e-4, max_rounds=32)
    vp = _params(pkg, f)
    raw = _records(f.rt, 48)
    iraw = _info_records(f.info, 288)
    d_pose, d_info = torch.from_numpy(raw.reshape(-1).copy()).cuda(), torch.from_numpy(iraw.reshape(-1).copy()).cuda()
    d_sset = torch.full((f.n_sets * 160,), 0xAB, dtype=torch.uint8, device="cuda")
    d_spair = torch.full((P * 32,), 0xAC, dtype=torch.uint8, device="cuda")
    d_ssum = torch.full((32,), 0xCD, dtype=torch.uint8, device="cuda")
    d_set, d_pair, d_sum = _outputs(f.n_sets, P)
    torch.cuda.synchronize()
    reg.pairs_sync_device(f.n_sets, f.pairs, sp, d_pose.data_ptr(), 48, 0, 4, 0, d_sset.data_ptr(), d_spair.data_ptr(), d_ssum.data_ptr())
    reg.pairs_solve_device(f.n_sets, f.pairs, vp, d_pose.data_ptr(), 48, 0, 4, d_info.data_ptr(), 288, d_sset.data_ptr(), 160, d_set.data_ptr(),
                           d_pair.data_ptr(), d_sum.data_ptr())
    torch.cuda.synchronize()
    thr = pkg.sync_thresholds(sp)
    ssets, _sres, _ssum = SR.sync(f.n_sets, f.pairs, f.rt, thr[0], thr[1], max_rounds=32)
    assert d_sset.cpu().numpy().tobytes() == ssets.tobytes()
    init = (ssets["X"], ssets["status"])
    exp = _expected(pkg, f, vp, init)
    got = _fetch(pkg, d_set, d_pair, d_sum)
    _assert_same(got, exp, name + ", chained")
    assert int(got[2]["stop"]) == pkg.SC_SOLVE_STOP_CONVERGED and float(got[2]["cost"]) < float(got[2]["cost0"])
    host = reg.pairs_solve(f.n_sets, f.pairs, f.rt, ssets, vp, info=f.info)
    _assert_same(host, exp, name + ", host form")
    # behind itself: the call's own set records are a start
    again = reg.pairs_solve(f.n_sets, f.pairs, f.rt, host[0], vp, info=f.info)
    _assert_same(again, _expected(pkg, f, vp, (exp[0]["X"], exp[0]["status"])), name + ", behind itself")


# 3. the whole chain on one stream: register -> pose info -> cycles -> sync -> solve
def test_the_whole_chain_on_one_stream(pkg, reg):
    import torch
    rng = np.random.default_rng(864)
    n, S, knn, tau = 64, 8, 1, 0.02
    base, feat = rng.uniform(-1, 1, (n, 3)), rng.normal(size=(n, 33))
    R, t = CR.absolute_poses(S, 865)
    # (the rows of a set are permuted, its descriptors with them)
    pts, fts = [], []
    for s in range(S):
        perm = rng.permutation(n)
        pts.append(((base - t[s]) @ R[s] + 0.001 * rng.normal(size=(n, 3)))[perm])
        fts.append((feat + 0.05 * rng.normal(size=(n, 33)))[perm])
    pts, fts = np.ascontiguousarray(np.concatenate(pts), np.float32), np.ascontiguousarray(np.concatenate(fts), np.float32)
    set_off = (np.arange(S + 1) * n).astype(np.uint32)
    pairs = np.array([(i, (i + 1) % S) for i in range(S)] + [((i + 2) % S, i) for i in range(S)], np.uint32)  # every pair lies in a triangle
    P = len(pairs)
    mp = pkg.api.make_match_params(33, knn=knn, mutual=True)
    p = pkg.make_params(**dict(M.KW, tau=tau))
    cp = pkg.make_cycle_params(rot_tol=0.05, trans_tol=0.05)
    sp = pkg.make_sync_params(1e-4, 1e-4, flags=pkg.SC_SYNC_STATUS)
    vp = pkg.make_solve_params(1e-6, 1e-6, 1e-3, flags=pkg.SC_SOLVE_STATUS | pkg.SC_SOLVE_INFO_STATUS)
    slot = reg.pairs_layout(set_off, pairs, knn)
    slots = int(slot[-1])
    d_pts, d_feat = torch.from_numpy(pts).cuda(), torch.from_numpy(fts).cuda()
    d_res = torch.zeros(P * 80, dtype=torch.uint8, device="cuda")
    d_corr = torch.full((slots, 2), -7, dtype=torch.int32, device="cuda"); d_d2 = torch.zeros(slots, dtype=torch.float32, device="cuda")
    d_count = torch.full((P, 2), 9, dtype=torch.int32, device="cuda"); d_mask = torch.zeros(slots, dtype=torch.uint8, device="cuda")
    d_info = torch.full((P * 320,), 0xA5, dtype=torch.uint8, device="cuda")
    d_cres = torch.full((P * 48,), 0xAB, dtype=torch.uint8, device="cuda"); d_csum = torch.full((32,), 0xCD, dtype=torch.uint8, device="cuda")
    d_sset = torch.full((S * 160,), 0xAB, dtype=torch.uint8, device="cuda"); d_spair = torch.full((P * 32,), 0xAC, dtype=torch.uint8, device="cuda")
    d_ssum = torch.full((32,), 0xCD, dtype=torch.uint8, device="cuda")
    d_set, d_pair, d_sum = _outputs(S, P)
    alive_at = pkg.CYCLE_RESULT_DTYPE.fields["alive"][1]
    torch.cuda.synchronize()
    reg.register_pairs_features_device(d_pts.data_ptr(), d_feat.data_ptr(), set_off, pairs, mp, p, d_res.data_ptr(), d_corr.data_ptr(), d_d2.data_ptr(),
                                       d_count.data_ptr(), d_mask.data_ptr())
    reg.pose_info_pairs_slots_device(d_pts.data_ptr(), set_off, pairs, knn, p, d_corr.data_ptr(), d_count.data_ptr(), d_res.data_ptr(), 80, d_info.data_ptr())
    reg.pairs_cycles_device(S, pairs, cp, d_res.data_ptr(), 80, 0, d_cres.data_ptr(), d_csum.data_ptr())
    reg.pairs_sync_device(S, pairs, sp, d_res.data_ptr(), 80, d_cres.data_ptr() + alive_at, 48, 0, d_sset.data_ptr(), d_spair.data_ptr(), d_ssum.data_ptr())
    reg.pairs_solve_device(S, pairs, vp, d_res.data_ptr(), 80, d_cres.data_ptr() + alive_at, 48, d_info.data_ptr(), 320, d_sset.data_ptr(), 160,
                           d_set.data_ptr(), d_pair.data_ptr(), d_sum.data_ptr())
    torch.cuda.synchronize()
    got = _fetch(pkg, d_set, d_pair, d_sum)
    # the host forms one by one, on the records the first two stages left
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE)
    info = np.frombuffer(d_info.cpu().numpy().tobytes(), pkg.POSE_INFO_RESULT_DTYPE)
    assert (res["status"] == SC_OK).sum() >= P - 2 and (info["status"] == SC_OK).sum() >= P - 2
    cres, _csum = reg.pairs_cycles(S, pairs, res, cp)
    ssets, _sres, _ssum = reg.pairs_sync(S, pairs, res, sp, use=cres)
    assert d_sset.cpu().numpy().tobytes() == ssets.tobytes()
    host = reg.pairs_solve(S, pairs, res, ssets, vp, use=cres, info=info)
    _assert_same(got, host, "the chain against the host forms")
    # ... and the reference on the same records
    f = V.Family(S, pairs, res["Rt"], info["info"])
    f.statuses, f.info_statuses, f.use = res["status"].copy(), info["status"].copy(), cres["alive"].copy()
    _assert_same(got, _expected(pkg, f, vp, (ssets["X"], ssets["status"])), "the chain against the reference")
    assert int(got[2]["used_pairs"]) >= P - 2 and int(got[2]["stop"]) in (pkg.SC_SOLVE_STOP_CONVERGED, pkg.SC_SOLVE_STOP_ROSE)
    assert float(got[2]["cost"]) <= float(got[2]["cost0"])


# 4. the loop trips: a hub's list past one and two trips of the lane loop; sets past one chunk, and many chunks
@pytest.mark.parametrize("n", [66, 130])
def test_a_hub_past_a_trip_of_the_lane_loop(pkg, reg, n):
    f = V.hub(n)
    assert (f.pairs == 0).any(axis=1).sum() == n - 1  # 65 and 129 entries in set 0's list
    for anchor in (0, 7):  # the hub fixed, and the hub a set like any other
        got, _exp = _both(pkg, reg, f, f"hub({n}), anchor {anchor}", anchor=anchor)
        assert int(got[2]["free_sets"]) == n - 1 and int(got[2]["inner_total"]) > 0


@pytest.mark.parametrize("n", [65, 4097])
def test_sets_past_a_chunk(pkg, reg, n):
    f = V.lattice(n)
    got, _exp = _both(pkg, reg, f, f"lattice({n})")
    assert int(got[2]["free_sets"]) == n - 1 and int(got[2]["used_pairs"]) == 2 * n and float(got[2]["cost"]) < float(got[2]["cost0"])


# 5. every stop reason, by name
def test_stop_reasons(pkg, reg):
    f = V.k24()
    got, _ = _both(pkg, reg, f, "converged")
    assert int(got[2]["stop"]) == pkg.SC_SOLVE_STOP_CONVERGED and 1 < int(got[2]["outer"]) < 8
    got, _ = _both(pkg, reg, f, "max_outer 1", max_outer=1)
    assert (int(got[2]["stop"]), int(got[2]["outer"])) == (pkg.SC_SOLVE_STOP_MAX_OUTER, 1)
    got, _ = _both(pkg, reg, f, "max_inner 1", max_inner=1)
    assert int(got[2]["inner_last"]) == 1 and int(got[2]["inner_total"]) == int(got[2]["outer"])
    got, _ = _both(pkg, reg, f, "cg_tol 0", cg_tol=0.0, max_outer=2)
    assert int(got[2]["inner_last"]) > 13  # (13 at 1e-3: tests/test_solve_abi.py)
    g = V.k24(V.ROSE_RAD, V.ROSE_TRANS)
    got, _ = _both(pkg, reg, g, "rose", max_outer=32, rot_tol=0.0, trans_tol=0.0)
    assert int(got[2]["stop"]) == pkg.SC_SOLVE_STOP_ROSE and int(got[2]["outer"]) >= 1


# 6. the edge inputs
def test_edge_inputs(pkg, reg):
    f = V.edges()
    init = (f.init_X, f.init_status)
    got, exp = _both(pkg, reg, f, "edges", init=init)
    sets, res, s = got
    assert sets["state"][[3, 5, 7]].tolist() == [pkg.SC_SOLVE_ANCHOR, pkg.SC_SOLVE_UNKNOWN, pkg.SC_SOLVE_UNKNOWN]
    assert sets["X"][3].tobytes() == f.init_X[3].tobytes() and sets["X"][3][:9].tolist() != [1, 0, 0, 0, 1, 0, 0, 0, 1]  # the anchor keeps its X
    assert sets["X"][[5, 7]].tobytes() == f.init_X[[5, 7]].tobytes() and sets["status"][5] == SC_ENOHYP  # passed through, NaN and all
    assert np.isfinite(np.delete(sets["X"], 7, axis=0)).all()
    assert res["status"][[10, 11, 12]].tolist() == [SC_EINVAL, SC_ENOHYP, SC_OK] and not res["used"][[10, 11, 12, 15, 16, 17]].any()
    assert res["used"][13] == 1 and res["used"][14] == 1  # the repeated pair counts twice
    touching = ((f.pairs == 5) | (f.pairs == 7)).any(axis=1)
    assert not res["used"][touching].any() and int(s["used_pairs"]) == int(res["used"].sum()) and int(s["free_sets"]) == 21
    _assert_same(_host(pkg, reg, f, _params(pkg, f), init), exp, "edges, host form")
    # without the flags the words at bytes 48 and 296 are not statuses
    g = V.edges(); g.params["flags"] = 0
    vp = _params(pkg, g)
    e2 = _expected(pkg, g, vp, init)
    _assert_same(_device(pkg, reg, g, vp, init, pose_stride=64, info_stride=320), e2, "the statuses are not read")
    assert e2[1]["used"][11] == 1 and e2[1]["used"][17] == 1
    # other strides
    _assert_same(_device(pkg, reg, f, _params(pkg, f), init, pose_stride=80, info_stride=304, use_stride=12, init_stride=176), exp, "other strides")


def test_a_held_set_and_a_floating_component(pkg, reg):
    f = V.held()
    got, _ = _both(pkg, reg, f, "held")
    sets, _res, s = got
    X0, _st = V.sync_start(f)
    assert int(s["held_last"]) == 1 and int(sets["degenerate"][4]) == int(s["outer"]) and sets["state"][4] == pkg.SC_SOLVE_FREE
    assert sets["X"][4].tobytes() == X0[4].tobytes()  # held: it did not move
    g = V.floating()
    got, _ = _both(pkg, reg, g, "floating", init=(g.init_X, g.init_status))
    assert int(got[2]["free_sets"]) == 29 and int(got[2]["stop"]) == pkg.SC_SOLVE_STOP_CONVERGED and np.isfinite(got[0]["X"]).all()
    assert (got[0]["X"][24:] != g.init_X[24:]).any()  # the floating component moved, in its own gauge


def test_a_null_info_equals_identity_records(pkg, reg):
    f = V.k24(info=False)
    vp = _params(pkg, f)
    init = V.sync_start(f)
    null = _device(pkg, reg, f, vp, init)
    ident = _device(pkg, reg, f, vp, init, identity_records=True)
    _assert_same(null, ident, "NULL against identity records")
    _assert_same(null, _expected(pkg, f, vp, init), "NULL against the reference")


def test_no_free_set(pkg, reg):
    f = V.Family(3, [(0, 1), (2, 2)], np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (2, 1)))
    X0 = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0, 0], np.float64), (3, 1))
    init = (X0, np.array([SC_OK, SC_ENOHYP, SC_OK], np.int32))  # the anchor, an unknown set, an isolated one
    got, _ = _both(pkg, reg, f, "no free set", init=init)
    assert (int(got[2]["outer"]), int(got[2]["stop"]), int(got[2]["free_sets"]), int(got[2]["used_pairs"])) == (0, pkg.SC_SOLVE_STOP_CONVERGED, 0, 0)
    assert got[0]["state"].tolist() == [pkg.SC_SOLVE_ANCHOR, pkg.SC_SOLVE_UNKNOWN, pkg.SC_SOLVE_ISOLATED] and got[0]["X"].tobytes() == X0.tobytes()


# 7. the call sequence: two calls with no wait between them; a second call on a smaller list
def test_two_calls_with_no_wait_and_a_smaller_list(pkg, reg):
    import torch
    big, small = V.k24(), V.held()
    runs = []
    for f in (big, small):
        vp = _params(pkg, f)
        init = V.sync_start(f)
        d = dict(f=f, vp=vp, init=init, pose=torch.from_numpy(_records(f.rt, 48).reshape(-1).copy()).cuda(),
                 info=torch.from_numpy(_info_records(f.info, 288).reshape(-1).copy()).cuda(),
                 start=torch.from_numpy(_init_records(*init).reshape(-1).copy()).cuda(), out=_outputs(f.n_sets, len(f.pairs)))
        runs.append(d)
    torch.cuda.synchronize()
    for d in runs:
        f = d["f"]
        reg.pairs_solve_device(f.n_sets, f.pairs, d["vp"], d["pose"].data_ptr(), 48, 0, 4, d["info"].data_ptr(), 288, d["start"].data_ptr(), 160,
                               d["out"][0].data_ptr(), d["out"][1].data_ptr(), d["out"][2].data_ptr())
    torch.cuda.synchronize()
    for d in runs:
        _assert_same(_fetch(pkg, *d["out"]), _expected(pkg, d["f"], d["vp"], d["init"]), f"{d['f'].n_sets} sets, no wait between the calls")
    fresh = pkg.Registrar(0)
    try:
        first = _device(pkg, fresh, small, runs[1]["vp"], runs[1]["init"])
    finally:
        fresh.close()
    _assert_same(_fetch(pkg, *runs[1]["out"]), first, "a second call on a smaller list equals a fresh context's")


def _scene(pkg, n=300):
    sc = MR.scene(pkg, n)
    return sc.src, sc.tgt, pkg.make_params(**MR.kw_of())


# 8. the context rules
def test_the_workspace_of_a_context_that_never_calls_the_entry(pkg):
    src, tgt, p = _scene(pkg, 200)
    a, b = pkg.Registrar(0), pkg.Registrar(0)
    try:
        wa = a.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        wb = b.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        assert wa == wb > 0
        g = SR.k24()
        ssets, _r, _s = b.pairs_sync(g.n_sets, g.pairs, g.rt, pkg.make_sync_params(1e-4, 1e-4))
        with_sync = b.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        f = V.k24()
        b.pairs_solve(f.n_sets, f.pairs, f.rt, ssets, _params(pkg, f), info=f.info)
        assert a.register(src, tgt, params=p)["stats"]["workspace_bytes"] == wa  # unchanged where the entry is never called
        grown = b.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        assert grown >= with_sync + 276 * (32 + 16 + 584) + 25 * 4 + 24 * 664 + 19456  # ... and counted where it is
    finally:
        a.close(); b.close()


def test_the_entry_ends_a_frame_and_refuses_an_outstanding_call(pkg, reg):
    import torch
    src, tgt, p = _scene(pkg)
    f = V.held()
    init = np.frombuffer(_init_records(*V.sync_start(f)).tobytes(), pkg.SYNC_SET_DTYPE)
    assert reg.register(src, tgt, params=p)["status"] == SC_OK
    reg.pairs_solve(f.n_sets, f.pairs, f.rt, init, _params(pkg, f), info=f.info)
    with pytest.raises(pkg.SacCotError, match="no frame on this context"):
        reg.peel()
    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    d_Rt, d_mask = torch.zeros(12, device="cuda"), torch.zeros(len(src), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reg.register_device_async(d_src.data_ptr(), d_tgt.data_ptr(), len(src), p, d_Rt.data_ptr(), d_mask.data_ptr())
    try:
        with pytest.raises(pkg.SacCotError, match="a call is outstanding on this context"):
            reg.pairs_solve(f.n_sets, f.pairs, f.rt, init, _params(pkg, f), info=f.info)
    finally:
        rc, _ = reg.wait()
    assert rc == SC_OK


def test_every_refusal_names_its_rule(pkg, reg):
    f = V.held()
    L, h = pkg.load_library(), reg._h
    raw, iraw = _records(f.rt, 64), _info_records(f.info, 320)
    init = _init_records(*V.sync_start(f))
    sets, res, summ = np.zeros(5, pkg.SOLVE_SET_DTYPE), np.zeros(5, pkg.SOLVE_PAIR_DTYPE), np.zeros(1, pkg.SOLVE_SUMMARY_DTYPE)
    pairs = np.ascontiguousarray(f.pairs, np.uint32).reshape(-1)
    use = np.ones(5, np.uint32)
    vp_ = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731

    def call(n_sets=5, prs=pairs, n_pairs=5, sp=None, pose=raw, stride=64, u=None, use_stride=4, info=iraw, info_stride=320, ini=init, init_stride=160,
             s=sets, r=res, m=summ, device=False):
        sp = _params(pkg, f) if sp is None else sp  # (False: a NULL parameter block)
        fn = L.sc_pairs_solve_device if device else L.sc_pairs_solve
        rc = fn(h, n_sets, None if prs is None else u32(prs), n_pairs, None if sp is False else C.byref(sp), None if pose is None else vp_(pose), stride,
                None if u is None else vp_(u), use_stride, None if info is None else vp_(info), info_stride, None if ini is None else vp_(ini),
                init_stride, None if s is None else vp_(s), None if r is None else vp_(r), None if m is None else vp_(m))
        return rc, L.sc_last_error(h).decode()

    def refused(text, **kw):
        for device in (False, True):  # (every refusal comes before anything is enqueued: the device form never reads the host arrays it is handed here)
            rc, msg = call(device=device, **kw)
            assert rc == SC_EINVAL and text in msg and msg.startswith("sc_pairs_solve_device: " if device else "sc_pairs_solve: "), (kw, rc, msg)

    assert call()[0] == SC_OK and call(u=use)[0] == SC_OK and call(info=None)[0] == SC_OK
    for null in ("prs", "pose", "ini", "s", "r", "m"):
        refused("a NULL argument", **{null: None})
    refused("a NULL argument", sp=False)
    refused("n_sets == 0", n_sets=0)
    refused("n_pairs == 0", n_pairs=0)
    refused("n_pairs exceeds SC_CYCLES_MAX_PAIRS", n_pairs=(1 << 22) + 1)
    refused("a pair names a set index >= n_sets", n_sets=4)
    star = np.zeros((65536, 2), np.uint32); star[:, 1] = np.arange(1, 65537)
    refused("more than SC_CYCLES_MAX_DEGREE", n_sets=65537, prs=star.reshape(-1), n_pairs=65536)
    wrong = _params(pkg, f); wrong.size = 28
    refused("params->size", sp=wrong)
    refused("max_outer must be 1 .. 32", sp=_params(pkg, f, max_outer=0))
    refused("max_outer must be 1 .. 32", sp=_params(pkg, f, max_outer=33))
    refused("max_inner must be 1 .. 256", sp=_params(pkg, f, max_inner=0))
    refused("max_inner must be 1 .. 256", sp=_params(pkg, f, max_inner=257))
    refused("max_outer * max_inner must not exceed 2048", sp=_params(pkg, f, max_outer=9, max_inner=256))
    refused("rot_tol", sp=_params(pkg, f, rot_tol=3.2))
    refused("rot_tol", sp=_params(pkg, f, rot_tol=float("nan")))
    refused("trans_tol", sp=_params(pkg, f, trans_tol=-1.0))
    refused("trans_tol", sp=_params(pkg, f, trans_tol=float("inf")))
    refused("cg_tol", sp=_params(pkg, f, cg_tol=1.0))
    refused("cg_tol", sp=_params(pkg, f, cg_tol=-0.5))
    refused("cg_tol", sp=_params(pkg, f, cg_tol=float("nan")))
    refused("an unknown flag", sp=_params(pkg, f, flags=4))
    refused("pose_stride", stride=50)
    refused("pose_stride", stride=48, sp=_params(pkg, f, flags=pkg.SC_SOLVE_STATUS))
    refused("use_stride must be a multiple of 4 and at least 4", u=use, use_stride=0)
    refused("use_stride", u=use, use_stride=6)
    refused("info_stride must be a multiple of 8 and at least 288", info_stride=280)
    refused("info_stride", info_stride=292)
    refused("info_stride", info_stride=296, sp=_params(pkg, f, flags=pkg.SC_SOLVE_INFO_STATUS))
    refused("init_stride must be a multiple of 8 and at least 160", init_stride=152)
    refused("init_stride", init_stride=164)
    refused("anchor must be less than n_sets", sp=_params(pkg, f, anchor=5))
    assert call(use_stride=6)[0] == SC_OK and call(info=None, info_stride=7)[0] == SC_OK  # ignored without the array
    assert call(sp=_params(pkg, f, max_outer=8, max_inner=256))[0] == SC_OK  # 2048 exactly
    assert call()[0] == SC_OK  # the context is none the worse
