"""GPU: loop consistency of a pair list's poses (include/saccot.h, sc_pairs_cycles / sc_pairs_cycles_device).

The expected value of every case is tests/cycles_ref.py — numpy fp64 in the header's order, fed the two thresholds the library
itself derives (sc_cycles_thresholds) — and every comparison is bit for bit: the 48 bytes of every record, doubles included, and the
32 bytes of the summary.  min_trace and max_e2 are what pin the arithmetic.  No tolerances.
"""
import ctypes as C

import numpy as np
import pytest

import cycles_ref as CR
import merge_ref as MR

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
REC, SUM = 48, 32


def _params(pkg, f, **kw):
    p = dict(f.params); p.update(kw)
    return pkg.make_cycle_params(**p)


def _expected(pkg, f, cp, pairs=None, rt=None, keep=None, statuses=None):
    thr = pkg.cycles_thresholds(cp)
    return CR.cycles(f.n_sets, f.pairs if pairs is None else pairs, f.rt if rt is None else rt, thr[0], thr[1], min_ok=cp.min_ok,
                     max_rounds=cp.max_rounds, keep=keep, statuses=statuses)


def _assert_same(got, exp, what=""):
    (gr, gs), (er, es) = got, exp
    print(what, "summary", gs, "expected", es, "min_trace", gr["min_trace"].min(), er["min_trace"].min(), "max_e2", gr["max_e2"].max(), er["max_e2"].max(),
          "records that differ", int((gr.view(np.uint8).reshape(-1, REC) != er.view(np.uint8).reshape(-1, REC)).any(axis=1).sum()))
    assert np.asarray(gs).tobytes() == np.asarray(es).tobytes(), what
    for name in er.dtype.names:
        assert gr[name].tobytes() == er[name].tobytes(), (what, name)
    assert gr.tobytes() == er.tobytes(), what


def _records(rt, stride, statuses=None):
    """the poses as records of `stride` bytes: Rt at byte 0, the status at byte 48 where there is room, 0xA5 elsewhere"""
    raw = np.full((len(rt), stride), 0xA5, np.uint8)
    raw[:, :48] = np.ascontiguousarray(rt, np.float32).view(np.uint8).reshape(len(rt), 48)
    if stride >= 52:
        st = np.zeros(len(rt), np.int32) if statuses is None else np.asarray(statuses, np.int32)
        raw[:, 48:52] = st.view(np.uint8).reshape(len(rt), 4)
    return raw


def _device(pkg, r, n_sets, pairs, cp, raw, keep=None):
    """the device form on host data: copies in, one call, one device-wide wait -> (records, summary); the outputs are pre-filled
    with sentinel bytes"""
    import torch
    P, stride = raw.shape
    d_pose = torch.from_numpy(raw.reshape(-1).copy()).cuda()
    d_keep = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).cuda()
    d_res = torch.full((P * REC,), 0xAB, dtype=torch.uint8, device="cuda")
    d_sum = torch.full((SUM,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.pairs_cycles_device(n_sets, pairs, cp, d_pose.data_ptr(), stride, 0 if d_keep is None else d_keep.data_ptr(), d_res.data_ptr(), d_sum.data_ptr())
    torch.cuda.synchronize()
    assert d_pose.cpu().numpy().tobytes() == raw.tobytes()  # d_pose is read, never written
    return (np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.CYCLE_RESULT_DTYPE), np.frombuffer(d_sum.cpu().numpy().tobytes(), pkg.CYCLE_SUMMARY_DTYPE)[0])


def _host(pkg, r, n_sets, pairs, cp, raw, keep=None):
    rec = np.frombuffer(raw.tobytes(), np.dtype((np.void, raw.shape[1])))
    dt = np.dtype({"names": ["Rt"], "formats": [("<f4", (12,))], "offsets": [0], "itemsize": raw.shape[1]})
    return r.pairs_cycles(n_sets, pairs, rec.view(dt), cp, keep=keep)


@pytest.mark.parametrize("consistent", [True, False])
def test_one_triangle_in_every_stored_direction(pkg, reg, consistent):
    for directions in range(8):
        f = CR.one_triangle(directions, consistent)
        cp = _params(pkg, f)
        exp = _expected(pkg, f, cp)
        got = reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp)
        _assert_same(got, exp, f"directions {directions:03b}")
        assert (got[1]["triangles"], got[1]["consistent"], got[1]["alive"]) == (1, int(consistent), 3 if consistent else 0)
        _assert_same(_device(pkg, reg, f.n_sets, f.pairs, cp, _records(f.rt, 48)), exp, f"directions {directions:03b}, device form")


def test_set_indices_out_of_order(pkg, reg):
    """the three sets of a triangle are 9, 2 and 5 of twelve, and a second triangle shares a pair with it: the roles follow the set
    indices, not the list"""
    R, t = CR.absolute_poses(12, 21)
    pairs = np.array([(9, 2), (5, 9), (5, 2), (11, 2), (9, 11), (0, 7)])
    rt = CR.corrupt(CR.relative_poses(pairs, R, t), [3], 22)
    f = CR.Family(12, pairs, rt, rot_tol=CR.ROT_TOL, trans_tol=CR.TRANS_TOL)
    cp = _params(pkg, f)
    got = reg.pairs_cycles(12, pairs, rt, cp)
    _assert_same(got, _expected(pkg, f, cp), "out of order")
    assert got[0]["cycles"].tolist() == [2, 1, 1, 1, 1, 0] and got[0]["ok"].tolist() == [1, 1, 1, 0, 0, 0] and got[1]["alive"] == 3


@pytest.mark.parametrize("min_ok", [1, 3, 8])
def test_k24_equals_the_reference(pkg, reg, min_ok):
    f = CR.k24()
    st = np.zeros(len(f.pairs), np.int32)
    for stride in (48, 64, 80):
        for flags in ((0,) if stride == 48 else (0, pkg.SC_CYCLES_STATUS)):
            cp = _params(pkg, f, min_ok=min_ok, flags=flags)
            exp = _expected(pkg, f, cp, statuses=st if flags else None)
            raw = _records(f.rt, stride)
            _assert_same(_device(pkg, reg, f.n_sets, f.pairs, cp, raw), exp, f"device form, stride {stride}, flags {flags}")
            _assert_same(_host(pkg, reg, f.n_sets, f.pairs, cp, raw), exp, f"host form, stride {stride}, flags {flags}")
    assert (exp[1]["rounds"], exp[1]["stable"], exp[1]["alive"], exp[1]["triangles"], exp[1]["consistent"]) == (2, 1, 248, 2024, 1476)
    # without the flag the word at byte 48 is not a status: 0xA5A5A5A5 there changes nothing (checked above at strides 64 and 80)


@pytest.mark.parametrize("max_rounds", [64, 5])
def test_the_strip(pkg, reg, max_rounds):
    f = CR.strip()
    cp = _params(pkg, f, max_rounds=max_rounds)
    exp = _expected(pkg, f, cp, keep=f.keep)
    _assert_same(reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp, keep=f.keep), exp, f"host form, max_rounds {max_rounds}")
    _assert_same(_device(pkg, reg, f.n_sets, f.pairs, cp, _records(f.rt, 48), keep=f.keep), exp, f"device form, max_rounds {max_rounds}")
    assert (exp[1]["rounds"], exp[1]["stable"]) == ((41, 1) if max_rounds == 64 else (5, 0))
    assert (exp[0]["dropped_round"] > 0).sum() == (40 if max_rounds == 64 else 5)
    # the same list without the keep bytes (NULL): whatever it unravels to, it is the reference's
    _assert_same(reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp), _expected(pkg, f, cp), "no keep")


def test_min_ok_zero_is_one_round_and_drops_nothing(pkg, reg):
    f = CR.k24()
    cp = _params(pkg, f, min_ok=0)
    got = reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp)
    _assert_same(got, _expected(pkg, f, cp), "min_ok 0")
    assert (got[1]["rounds"], got[1]["stable"], got[1]["alive"]) == (1, 1, 276) and not got[0]["dropped_round"].any()
    assert (got[0]["ok_alive"] == got[0]["ok"]).all()


def test_repeated_and_reversed_pairs(pkg, reg):
    f = CR.k24_repeats()
    cp = _params(pkg, f, min_ok=3)
    exp = _expected(pkg, f, cp)
    got = reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp)
    _assert_same(got, exp, "repeats")
    assert got[1]["triangles"] > 2024 and got[0]["cycles"].max() > 22
    _assert_same(_device(pkg, reg, f.n_sets, f.pairs, cp, _records(f.rt, 64)), exp, "repeats, device form")


def test_self_pairs_and_invalid_poses_take_part_in_nothing(pkg, reg):
    f = CR.k24()
    P = len(f.pairs)
    pairs = f.pairs.copy(); pairs[11] = (7, 7); pairs[200] = (0, 0)
    rt = f.rt.copy(); rt[5, 3] = np.nan; rt[6, 10] = np.inf
    st = np.zeros(P, np.int32); st[9] = SC_ENOHYP; st[5] = 0
    out = [5, 6, 9, 11, 200]
    cp = _params(pkg, f, flags=pkg.SC_CYCLES_STATUS)
    exp = _expected(pkg, f, cp, pairs=pairs, rt=rt, statuses=st)
    got = _device(pkg, reg, f.n_sets, pairs, cp, _records(rt, 64, st))
    _assert_same(got, exp, "invalid pairs")
    assert got[0]["status"][out].tolist() == [SC_EINVAL, SC_EINVAL, SC_ENOHYP, SC_OK, SC_OK] and got[1]["edges"] == P - 5
    for name in ("cycles", "ok", "ok_alive", "alive", "dropped_round", "max_e2"):
        assert not got[0][name][out].any(), name
    assert (got[0]["min_trace"][out] == 3.0).all()
    # the other pairs' records are those of the list without the five
    others = np.setdiff1d(np.arange(P), out)
    alone = _device(pkg, reg, f.n_sets, pairs[others], cp, _records(rt[others], 64))
    assert alone[0].tobytes() == got[0][others].tobytes() and alone[1].tobytes() == got[1].tobytes()
    # a status that is SC_OK with a pose that is not finite is SC_EINVAL; without the flag the status word is not read
    plain = _params(pkg, f)
    st_all = np.full(P, SC_ENOHYP, np.int32)
    _assert_same(_device(pkg, reg, f.n_sets, f.pairs, plain, _records(f.rt, 64, st_all)), _expected(pkg, f, plain), "the status is not read")


def test_a_hub_whose_list_is_longer_than_a_workgroup(pkg, reg):
    f = CR.hub()
    cp = _params(pkg, f)
    exp = _expected(pkg, f, cp)
    got = reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp)
    _assert_same(got, exp, "hub")
    assert got[1]["triangles"] == 1498 and 0 < got[1]["consistent"] < 1498 and got[1]["stable"] == 1
    # ... and with every spoke listed three times, so that the runs of equal neighbours are long as well
    spokes = f.pairs[:1499]
    pairs = np.concatenate([f.pairs, spokes[:, ::-1], spokes])
    R, t = CR.absolute_poses(f.n_sets, 11)
    rt = np.concatenate([f.rt, CR.relative_poses(spokes[:, ::-1], R, t), f.rt[:1499]])
    g = CR.Family(f.n_sets, pairs, rt, rot_tol=CR.ROT_TOL, trans_tol=CR.TRANS_TOL)
    cp = _params(pkg, g, min_ok=2)
    got = reg.pairs_cycles(g.n_sets, g.pairs, g.rt, cp)
    _assert_same(got, _expected(pkg, g, cp), "hub, spokes three times")
    assert got[1]["triangles"] == 9 * 1498 and got[0]["cycles"].max() == 9


def test_the_list_shuffled(pkg, reg):
    f = CR.k24_repeats()
    cp = _params(pkg, f, min_ok=3)
    base = reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp)
    perm = np.random.default_rng(17).permutation(len(f.pairs))
    got = reg.pairs_cycles(f.n_sets, f.pairs[perm], f.rt[perm], cp)
    assert got[0].tobytes() == base[0][perm].tobytes() and got[1].tobytes() == base[1].tobytes()


def test_two_calls_on_one_context_with_different_lists(pkg, reg):
    big, small = CR.hub(), CR.one_triangle(5, True)
    for f in (small, big, small, CR.k24(), small):
        cp = _params(pkg, f)
        _assert_same(_device(pkg, reg, f.n_sets, f.pairs, cp, _records(f.rt, 48)), _expected(pkg, f, cp), f"{len(f.pairs)} pairs")


def _scene(pkg, n=300):
    sc = MR.scene(pkg, n)
    return sc.src, sc.tgt, pkg.make_params(**MR.kw_of())


def test_the_entry_ends_a_frame(pkg, reg):
    src, tgt, p = _scene(pkg)
    assert reg.register(src, tgt, params=p)["status"] == SC_OK
    assert reg.peel()["status"] in (SC_OK, SC_ENOHYP)  # the frame is there
    assert reg.register(src, tgt, params=p)["status"] == SC_OK
    f = CR.one_triangle(0, True)
    reg.pairs_cycles(f.n_sets, f.pairs, f.rt, _params(pkg, f))
    with pytest.raises(pkg.SacCotError, match="no frame on this context"):
        reg.peel()
    # a refused call ends it as well, as every batch entry's does
    assert reg.register(src, tgt, params=p)["status"] == SC_OK
    with pytest.raises(pkg.SacCotError, match="a pair names a set index >= n_sets"):
        reg.pairs_cycles(2, f.pairs, f.rt, _params(pkg, f))
    with pytest.raises(pkg.SacCotError, match="no frame on this context"):
        reg.peel()


def test_a_call_outstanding_is_refused(pkg, reg):
    import torch
    src, tgt, p = _scene(pkg)
    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    d_Rt, d_mask = torch.zeros(12, device="cuda"), torch.zeros(len(src), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    f = CR.one_triangle(0, True)
    reg.register_device_async(d_src.data_ptr(), d_tgt.data_ptr(), len(src), p, d_Rt.data_ptr(), d_mask.data_ptr())
    try:
        with pytest.raises(pkg.SacCotError, match="a call is outstanding on this context"):
            reg.pairs_cycles(f.n_sets, f.pairs, f.rt, _params(pkg, f))
    finally:
        rc, _ = reg.wait()
    assert rc == SC_OK
    _assert_same(reg.pairs_cycles(f.n_sets, f.pairs, f.rt, _params(pkg, f)), _expected(pkg, f, _params(pkg, f)), "after the wait")


def test_the_workspace_of_a_context_that_never_calls_the_entry(pkg):
    """a fresh context that registers holds what it held before this entry existed: the entry's buffers come with its first call"""
    src, tgt, p = _scene(pkg, 200)
    a, b = pkg.Registrar(0), pkg.Registrar(0)
    try:
        wa = a.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        wb = b.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        assert wa == wb > 0
        f = CR.k24()
        b.pairs_cycles(f.n_sets, f.pairs, f.rt, _params(pkg, f))
        assert a.register(src, tgt, params=p)["stats"]["workspace_bytes"] == wa  # unchanged where the entry is never called
        grown = b.register(src, tgt, params=p)["stats"]["workspace_bytes"]
        assert grown >= wb + 276 * (32 + 16 + 192 + 2 + 48) + 32  # ... and counted where it is: meta, poses, alive bytes, the host form's copies
    finally:
        a.close(); b.close()


def test_every_refusal_names_its_rule(pkg, reg):
    f = CR.one_triangle(0, True)
    L, h = pkg.load_library(), reg._h
    raw = _records(f.rt, 64)
    res, summ = np.zeros(3, pkg.CYCLE_RESULT_DTYPE), np.zeros(1, pkg.CYCLE_SUMMARY_DTYPE)
    pairs = np.ascontiguousarray(f.pairs, np.uint32).reshape(-1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731

    def call(n_sets=3, prs=pairs, n_pairs=3, cp=None, pose=raw, stride=64, r=res, s=summ, device=False):
        cp = _params(pkg, f) if cp is None else cp  # (False: a NULL parameter block)
        fn = L.sc_pairs_cycles_device if device else L.sc_pairs_cycles
        rc = fn(h, n_sets, None if prs is None else u32(prs), n_pairs, None if cp is False else C.byref(cp), None if pose is None else vp(pose), stride, None,
                None if r is None else vp(r), None if s is None else vp(s))
        return rc, L.sc_last_error(h).decode()

    def refused(text, **kw):
        for device in (False, True):  # (every refusal comes before anything is enqueued: the device form never reads the host arrays it is handed here)
            rc, msg = call(device=device, **kw)
            assert rc == SC_EINVAL and text in msg and msg.startswith("sc_pairs_cycles_device: " if device else "sc_pairs_cycles: "), (kw, rc, msg)

    assert call()[0] == SC_OK
    for null in ("prs", "pose", "r", "s"):
        refused("a NULL argument", **{null: None})
    refused("a NULL argument", cp=False)
    refused("n_sets == 0", n_sets=0)
    refused("n_pairs == 0", n_pairs=0)
    refused("n_pairs exceeds SC_CYCLES_MAX_PAIRS", n_pairs=(1 << 22) + 1)
    refused("a pair names a set index >= n_sets", n_sets=2)
    star = np.zeros((65536, 2), np.uint32); star[:, 1] = np.arange(1, 65537)
    refused("more than SC_CYCLES_MAX_DEGREE", n_sets=65537, prs=star.reshape(-1), n_pairs=65536)
    wrong = _params(pkg, f); wrong.size = 28
    refused("params->size", cp=wrong)
    refused("max_rounds must be 1 .. 64", cp=_params(pkg, f, max_rounds=0))
    refused("max_rounds must be 1 .. 64", cp=_params(pkg, f, max_rounds=65))
    refused("rot_tol", cp=_params(pkg, f, rot_tol=3.2))
    refused("rot_tol", cp=_params(pkg, f, rot_tol=float("nan")))
    refused("trans_tol", cp=_params(pkg, f, trans_tol=-1.0))
    refused("trans_tol", cp=_params(pkg, f, trans_tol=float("inf")))
    refused("an unknown flag", cp=_params(pkg, f, flags=2))
    res9 = _params(pkg, f); res9.reserved[0] = 1
    refused("a reserved field", cp=res9)
    refused("pose_stride", stride=50)
    refused("pose_stride", stride=44)
    refused("pose_stride", stride=48, cp=_params(pkg, f, flags=pkg.SC_CYCLES_STATUS))
    assert call()[0] == SC_OK  # the context is none the worse
