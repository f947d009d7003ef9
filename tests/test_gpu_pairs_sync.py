"""GPU: absolute poses of a pair list's sets (include/saccot.h, sc_pairs_sync / sc_pairs_sync_device).

The expected value of every case is tests/sync_ref.py — numpy fp64 in the header's order, the 64 slots and the fold restated
literally, fed the two thresholds the library itself derives (sc_sync_thresholds) — and every comparison is bit for bit: the 160
bytes of every set's record, the 32 of every pair's and the 32 of the summary, doubles compared as their bytes.  No tolerances.
"""
import ctypes as C

import numpy as np
import pytest

import cycles_ref as CR
import merge_ref as MR
import sync_ref as SR

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
SET, PAIR, SUM = 160, 32, 32


def _params(pkg, f, **kw):
    p = dict(f.params); p.update(kw)
    return pkg.make_sync_params(**p)


def _expected(pkg, f, sp, pairs=None, rt=None, use=None, weight=None, statuses=None):
    thr = pkg.sync_thresholds(sp)
    return SR.sync(f.n_sets, f.pairs if pairs is None else pairs, f.rt if rt is None else rt, thr[0], thr[1], anchor=sp.anchor,
                   max_rounds=sp.max_rounds, use=use, weight=weight, statuses=statuses)


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


def _fetch(pkg, d_set, d_pair, d_sum):
    return (np.frombuffer(d_set.cpu().numpy().tobytes(), pkg.SYNC_SET_DTYPE), np.frombuffer(d_pair.cpu().numpy().tobytes(), pkg.SYNC_PAIR_DTYPE),
            np.frombuffer(d_sum.cpu().numpy().tobytes(), pkg.SYNC_SUMMARY_DTYPE)[0])


def _device(pkg, r, n_sets, pairs, sp, raw, use=None, use_stride=4, weight=None):
    """the device form on host data: copies in, one call, one device-wide wait -> (sets, pairs, summary); the outputs are pre-filled
    with sentinel bytes.  use: uint32 words, use_stride bytes apart (0xA5 between them)."""
    import torch
    P, stride = raw.shape
    d_pose = torch.from_numpy(raw.reshape(-1).copy()).cuda()
    d_use = None
    if use is not None:
        words = np.full((P, use_stride), 0xA5, np.uint8)
        words[:, :4] = np.ascontiguousarray(use, np.uint32).view(np.uint8).reshape(P, 4)
        d_use = torch.from_numpy(words.reshape(-1)).cuda()
    d_w = None if weight is None else torch.from_numpy(np.ascontiguousarray(weight, np.float32)).cuda()
    d_set = torch.full((n_sets * SET,), 0xAB, dtype=torch.uint8, device="cuda")
    d_pair = torch.full((P * PAIR,), 0xAC, dtype=torch.uint8, device="cuda")
    d_sum = torch.full((SUM,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.pairs_sync_device(n_sets, pairs, sp, d_pose.data_ptr(), stride, 0 if d_use is None else d_use.data_ptr(), use_stride,
                        0 if d_w is None else d_w.data_ptr(), d_set.data_ptr(), d_pair.data_ptr(), d_sum.data_ptr())
    torch.cuda.synchronize()
    assert d_pose.cpu().numpy().tobytes() == raw.tobytes()  # d_pose is read, never written
    return _fetch(pkg, d_set, d_pair, d_sum)


def _host(pkg, r, n_sets, pairs, sp, raw, use=None, weight=None):
    rec = np.frombuffer(raw.tobytes(), np.dtype((np.void, raw.shape[1])))
    dt = np.dtype({"names": ["Rt"], "formats": [("<f4", (12,))], "offsets": [0], "itemsize": raw.shape[1]})
    return r.pairs_sync(n_sets, pairs, rec.view(dt), sp, use=use, weight=weight)


# 1. k24, noisy, and with repeated pairs in both directions
def test_k24_equals_the_reference(pkg, reg):
    f = SR.k24()
    st = np.zeros(len(f.pairs), np.int32)
    for stride in (48, 64, 160):
        for flags in ((0,) if stride == 48 else (0, pkg.SC_SYNC_STATUS)):
            sp = _params(pkg, f, flags=flags)
            exp = _expected(pkg, f, sp, statuses=st if flags else None)
            _assert_same(_device(pkg, reg, f.n_sets, f.pairs, sp, _records(f.rt, stride)), exp, f"device form, stride {stride}, flags {flags}")
    assert (exp[2]["rounds"], exp[2]["converged"], exp[2]["known"], exp[2]["used"]) == (4, 1, 24, 276)
    g = SR.k24_repeats()
    sp = _params(pkg, g)
    exp = _expected(pkg, g, sp)
    _assert_same(_device(pkg, reg, g.n_sets, g.pairs, sp, _records(g.rt, 48)), exp, "repeats")
    assert exp[0]["used"].max() > 23 and exp[2]["used"] == 283


# 2. the chain: cycles then sync on one stream, nothing waited for in between
def test_cycles_then_sync_on_one_stream(pkg, reg):
    import torch
    f = CR.k24()  # 28 of its 276 poses are wrong
    P = len(f.pairs)
    cp = pkg.make_cycle_params(**f.params)
    sp = pkg.make_sync_params(SR.TOL, SR.TOL)
    raw = _records(f.rt, 64)
    d_pose = torch.from_numpy(raw.reshape(-1).copy()).cuda()
    d_res = torch.full((P * 48,), 0xAB, dtype=torch.uint8, device="cuda")
    d_csum = torch.full((32,), 0xCD, dtype=torch.uint8, device="cuda")
    d_set = torch.full((f.n_sets * SET,), 0xAB, dtype=torch.uint8, device="cuda")
    d_pair = torch.full((P * PAIR,), 0xAC, dtype=torch.uint8, device="cuda")
    d_sum = torch.full((SUM,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    alive_at = pkg.CYCLE_RESULT_DTYPE.fields["alive"][1]
    reg.pairs_cycles_device(f.n_sets, f.pairs, cp, d_pose.data_ptr(), 64, 0, d_res.data_ptr(), d_csum.data_ptr())
    reg.pairs_sync_device(f.n_sets, f.pairs, sp, d_pose.data_ptr(), 64, d_res.data_ptr() + alive_at, 48, 0, d_set.data_ptr(), d_pair.data_ptr(),
                          d_sum.data_ptr())
    torch.cuda.synchronize()
    thr = pkg.cycles_thresholds(cp)
    cyc = CR.cycles(f.n_sets, f.pairs, f.rt, thr[0], thr[1], min_ok=cp.min_ok, max_rounds=cp.max_rounds)
    assert d_res.cpu().numpy().tobytes() == cyc[0].tobytes() and alive_at == 16
    exp = _expected(pkg, f, sp, use=cyc[0]["alive"])
    got = _fetch(pkg, d_set, d_pair, d_sum)
    _assert_same(got, exp, "cycles then sync")
    assert not got[1]["used"][f.bad].any() and got[2]["used"] == P - 28 and got[2]["known"] == 24 and got[2]["converged"] == 1
    assert SR.errors(got[0], SR.k24(False))[0] < 1e-6  # without the 28 the exact records give the exact poses
    # the host form reads the same words out of the cycle records
    res, _summary = reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp)
    _assert_same(reg.pairs_sync(f.n_sets, f.pairs, f.rt, sp, use=res), exp, "host form over the cycle records")


# 3. past one trip of the lane loop (and four), and of the grid loop
def test_a_hub_and_a_list_past_the_grid(pkg, reg):
    f = SR.hub()
    assert f.n_sets == 300 and (f.pairs == 0).any(axis=1).sum() == 299 > 4 * 64
    sp = _params(pkg, f)
    exp = _expected(pkg, f, sp)
    _assert_same(_device(pkg, reg, f.n_sets, f.pairs, sp, _records(f.rt, 48)), exp, "hub(300)")
    assert exp[0]["used"][0] == 0 and exp[2]["known"] == 300
    sp = _params(pkg, f, anchor=7)  # ... and with the hub a set like any other: 299 live entries in five trips
    exp = _expected(pkg, f, sp)
    _assert_same(_device(pkg, reg, f.n_sets, f.pairs, sp, _records(f.rt, 48)), exp, "hub(300), anchor 7")
    assert exp[0]["used"][0] == 299
    g = SR.wide()  # SYNC_BLOCKS = 2048 workgroups of four waves: 8192 sets a trip
    assert g.n_sets == SR.WIDE_SETS > 2048 * 4
    sp = _params(pkg, g)
    exp = _expected(pkg, g, sp)
    _assert_same(_device(pkg, reg, g.n_sets, g.pairs, sp, _records(g.rt, 48)), exp, "wide")
    assert exp[2]["known"] == g.n_sets and (exp[0]["known_round"][8192:] > 0).all() and exp[0]["used"][16] == 5


# 4. the chain of 42
@pytest.mark.parametrize("max_rounds", [20, 41, 42])
def test_the_chain(pkg, reg, max_rounds):
    f = SR.chain()
    sp = _params(pkg, f, max_rounds=max_rounds)
    exp = _expected(pkg, f, sp)
    _assert_same(_device(pkg, reg, f.n_sets, f.pairs, sp, _records(f.rt, 48)), exp, f"max_rounds {max_rounds}")
    assert (exp[2]["rounds"], exp[2]["converged"], exp[2]["known"]) == {20: (20, 0, 21), 41: (41, 0, 42), 42: (42, 1, 42)}[max_rounds]


# 5. an anchor other than 0; 6. a self pair; 7. a NaN pose and a status; 8. the weights
def test_anchor_self_pair_invalid_poses_and_weights(pkg, reg):
    f = SR.k24()
    P = len(f.pairs)
    sp = _params(pkg, f, anchor=17)
    exp = _expected(pkg, f, sp)
    _assert_same(_device(pkg, reg, f.n_sets, f.pairs, sp, _records(f.rt, 48)), exp, "anchor 17")
    assert exp[0]["X"][17].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and exp[0]["known_round"][17] == 0
    rt = f.rt.copy(); rt[5, 3] = np.nan; rt[6, 10] = np.inf
    st = np.zeros(P, np.int32); st[9] = SC_ENOHYP
    pairs = f.pairs.copy(); pairs[11] = (7, 7); pairs[200] = (0, 0)
    use = np.ones(P, np.uint32); use[12] = 0; use[13] = 0x80000000
    w = np.ones(P, np.float32); w[14] = 0; w[15] = -1; w[16] = np.inf; w[17] = np.nan; w[18] = 2.5; w[19] = 1e-3; w[20:60] = np.linspace(0.1, 4, 40)
    sp = _params(pkg, f, flags=pkg.SC_SYNC_STATUS)
    exp = _expected(pkg, f, sp, pairs=pairs, rt=rt, use=use, weight=w, statuses=st)
    got = _device(pkg, reg, f.n_sets, pairs, sp, _records(rt, 64, st), use=use, use_stride=12, weight=w)
    _assert_same(got, exp, "invalid, unused and unweighted pairs")
    out = [5, 6, 9, 11, 200, 12, 14, 15, 16, 17]
    assert got[1]["status"][[5, 6, 9, 11, 200]].tolist() == [SC_EINVAL, SC_EINVAL, SC_ENOHYP, SC_OK, SC_OK] and not got[1]["used"][out].any()
    assert got[2]["used"] == P - len(out)
    _assert_same(_host(pkg, reg, f.n_sets, pairs, sp, _records(rt, 64, st), use=use, weight=w), exp, "the same, host form")
    # without the flag the word at byte 48 is not a status
    plain = _params(pkg, f)
    _assert_same(_device(pkg, reg, f.n_sets, f.pairs, plain, _records(f.rt, 64, np.full(P, SC_ENOHYP, np.int32))), _expected(pkg, f, plain), "the status is not read")


# 9. two components; 10. the degenerate pair of predictions
def test_two_components_and_the_degenerate_sum(pkg, reg):
    f = SR.two_components()
    for anchor in (0, 26):
        sp = _params(pkg, f, anchor=anchor)
        exp = _expected(pkg, f, sp)
        _assert_same(_device(pkg, reg, f.n_sets, f.pairs, sp, _records(f.rt, 48)), exp, f"two components, anchor {anchor}")
        assert exp[2]["known"] == (24 if anchor == 0 else 6)
    f = SR.degenerate()
    sp = _params(pkg, f)
    exp = _expected(pkg, f, sp)
    got = _device(pkg, reg, f.n_sets, f.pairs, sp, _records(f.rt, 48))
    _assert_same(got, exp, "degenerate")
    assert got[0]["degenerate"].tolist() == [0, 1, 0, 0] and got[0]["status"][1] == SC_ENOHYP and not got[0]["X"][1].any()


# 11. the cuts
def test_a_set_on_the_cut_is_quiet(pkg, reg):
    f = SR.cut24()
    below = float(np.nextafter(np.float32(SR.CUT_TOL), np.float32(0)))
    rounds = {}
    for tol in (SR.CUT_TOL, below):
        sp = _params(pkg, f, trans_tol=tol)
        assert pkg.sync_thresholds(sp) == SR.thresholds(0.0, tol)
        exp = _expected(pkg, f, sp, use=f.use)
        got = _device(pkg, reg, f.n_sets, f.pairs, sp, _records(f.rt, 48), use=f.use)
        _assert_same(got, exp, f"trans_tol {tol!r}")
        rounds[tol] = (int(got[2]["rounds"]), int(got[2]["converged"]))
    assert rounds == {SR.CUT_TOL: (2, 1), below: (3, 1)}  # (tests/test_sync_abi.py shows dt2 == e2_max == 2^-8 in round 2)


# 12. the host form; 13. a second call on the context against a fresh context
def test_the_host_form_and_a_second_call(pkg, reg):
    f = SR.g512()
    sp = _params(pkg, f)
    exp = _expected(pkg, f, sp)
    dev = _device(pkg, reg, f.n_sets, f.pairs, sp, _records(f.rt, 48))
    _assert_same(dev, exp, "g512, device form")
    _assert_same(_host(pkg, reg, f.n_sets, f.pairs, sp, _records(f.rt, 48)), exp, "g512, host form")
    _assert_same(reg.pairs_sync(f.n_sets, f.pairs, f.rt, sp), exp, "g512, host form, plain floats")
    small = SR.chain()
    sp2 = _params(pkg, small, max_rounds=64)
    second = _device(pkg, reg, small.n_sets, small.pairs, sp2, _records(small.rt, 48))  # after larger lists on the same context
    fresh = pkg.Registrar(0)
    try:
        first = _device(pkg, fresh, small.n_sets, small.pairs, sp2, _records(small.rt, 48))
    finally:
        fresh.close()
    _assert_same(second, first, "a second call equals a fresh context's")
    _assert_same(second, _expected(pkg, small, sp2), "the chain after g512")


def _scene(pkg, n=300):
    sc = MR.scene(pkg, n)
    return sc.src, sc.tgt, pkg.make_params(**MR.kw_of())


# 14. the workspace of a context that never calls the entry
def test_the_workspace_of_a_context_that_never_calls_the_entry(pkg):
    src, tgt, p = _scene(pkg, 200)
    a, b = pkg.Registrar(0), pkg.Registrar(0)
    try:
        wa = a.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        wb = b.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        assert wa == wb > 0
        f = CR.k24()
        b.pairs_cycles(f.n_sets, f.pairs, f.rt, pkg.make_cycle_params(**f.params))
        with_cycles = b.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        g = SR.k24()
        b.pairs_sync(g.n_sets, g.pairs, g.rt, _params(pkg, g))
        assert a.register(src, tgt, params=p)["stats"]["workspace_bytes"] == wa  # unchanged where the entry is never called
        grown = b.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        assert grown >= with_cycles + 276 * (32 + 16 + 200) + 25 * 4 + 2048 + 24 * 224  # ... and counted where it is: meta, poses, state
    finally:
        a.close(); b.close()


def test_the_entry_ends_a_frame_and_refuses_an_outstanding_call(pkg, reg):
    import torch
    src, tgt, p = _scene(pkg)
    f = SR.degenerate()
    assert reg.register(src, tgt, params=p)["status"] == SC_OK
    reg.pairs_sync(f.n_sets, f.pairs, f.rt, _params(pkg, f))
    with pytest.raises(pkg.SacCotError, match="no frame on this context"):
        reg.peel()
    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    d_Rt, d_mask = torch.zeros(12, device="cuda"), torch.zeros(len(src), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reg.register_device_async(d_src.data_ptr(), d_tgt.data_ptr(), len(src), p, d_Rt.data_ptr(), d_mask.data_ptr())
    try:
        with pytest.raises(pkg.SacCotError, match="a call is outstanding on this context"):
            reg.pairs_sync(f.n_sets, f.pairs, f.rt, _params(pkg, f))
    finally:
        rc, _ = reg.wait()
    assert rc == SC_OK


def test_every_refusal_names_its_rule(pkg, reg):
    f = SR.degenerate()
    L, h = pkg.load_library(), reg._h
    raw = _records(f.rt, 64)
    sets, res, summ = np.zeros(4, pkg.SYNC_SET_DTYPE), np.zeros(4, pkg.SYNC_PAIR_DTYPE), np.zeros(1, pkg.SYNC_SUMMARY_DTYPE)
    pairs = np.ascontiguousarray(f.pairs, np.uint32).reshape(-1)
    use = np.ones(4, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731

    def call(n_sets=4, prs=pairs, n_pairs=4, sp=None, pose=raw, stride=64, u=None, use_stride=4, s=sets, r=res, m=summ, device=False):
        sp = _params(pkg, f) if sp is None else sp  # (False: a NULL parameter block)
        fn = L.sc_pairs_sync_device if device else L.sc_pairs_sync
        rc = fn(h, n_sets, None if prs is None else u32(prs), n_pairs, None if sp is False else C.byref(sp), None if pose is None else vp(pose), stride,
                None if u is None else vp(u), use_stride, None, None if s is None else vp(s), None if r is None else vp(r), None if m is None else vp(m))
        return rc, L.sc_last_error(h).decode()

    def refused(text, **kw):
        for device in (False, True):  # (every refusal comes before anything is enqueued: the device form never reads the host arrays it is handed here)
            rc, msg = call(device=device, **kw)
            assert rc == SC_EINVAL and text in msg and msg.startswith("sc_pairs_sync_device: " if device else "sc_pairs_sync: "), (kw, rc, msg)

    assert call()[0] == SC_OK and call(u=use)[0] == SC_OK
    for null in ("prs", "pose", "s", "r", "m"):
        refused("a NULL argument", **{null: None})
    refused("a NULL argument", sp=False)
    refused("n_sets == 0", n_sets=0)
    refused("n_pairs == 0", n_pairs=0)
    refused("n_pairs exceeds SC_CYCLES_MAX_PAIRS", n_pairs=(1 << 22) + 1)
    refused("a pair names a set index >= n_sets", n_sets=3)
    star = np.zeros((65536, 2), np.uint32); star[:, 1] = np.arange(1, 65537)
    refused("more than SC_CYCLES_MAX_DEGREE", n_sets=65537, prs=star.reshape(-1), n_pairs=65536)
    wrong = _params(pkg, f); wrong.size = 28
    refused("params->size", sp=wrong)
    refused("max_rounds must be 1 .. 256", sp=_params(pkg, f, max_rounds=0))
    refused("max_rounds must be 1 .. 256", sp=_params(pkg, f, max_rounds=257))
    refused("rot_tol", sp=_params(pkg, f, rot_tol=3.2))
    refused("rot_tol", sp=_params(pkg, f, rot_tol=float("nan")))
    refused("trans_tol", sp=_params(pkg, f, trans_tol=-1.0))
    refused("trans_tol", sp=_params(pkg, f, trans_tol=float("inf")))
    refused("an unknown flag", sp=_params(pkg, f, flags=2))
    res9 = _params(pkg, f); res9.reserved[0] = 1
    refused("a reserved field", sp=res9)
    refused("pose_stride", stride=50)
    refused("pose_stride", stride=44)
    refused("pose_stride", stride=48, sp=_params(pkg, f, flags=pkg.SC_SYNC_STATUS))
    refused("use_stride must be a multiple of 4 and at least 4", u=use, use_stride=0)
    refused("use_stride", u=use, use_stride=6)
    refused("anchor must be less than n_sets", sp=_params(pkg, f, anchor=4))
    assert call(use_stride=6)[0] == SC_OK  # ignored without use
    assert call()[0] == SC_OK  # the context is none the worse
