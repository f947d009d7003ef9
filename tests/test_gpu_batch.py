"""GPU: many small registrations in one launch (include/saccot.h, sc_register_batch / sc_register_batch_device).

The expected value of every case is tests/batch_ref.py — problem b alone through the CPU restatement's whole path — and everything
is compared bit for bit: every field of every record and every mask byte.  Every problem holds at most batch_ref.TRI_CAP triangles
(asserted on the reference's counts), so no workgroup runs long.

Every scene here has unit extent.  tests/test_gpu_batch_range.py runs the same kernel, and its slot form, at the ends of the fp32
range, and puts the cut among equal keys on every boundary of the three find_cut passes (word, chunk, row and edge ends).
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref
import instances_batch_ref as IR
import match_batch_ref as M
import pairs_ref as P
import polish_batch_ref as PB
from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOMEM, SC_ENOHYP = 0, -1, -2, -5
SC_FLAG_TIMING, SC_FLAG_EXACT_TOTAL, SC_FLAG_REFINE = 1, 2, 8
FIELDS = ("status", "n", "edges", "tri_kept", "tri_total", "best_rank", "best_count")

_REF = {}


def _ref(O, tag, problems, kw, mode=0):
    """The reference of a set of problems, once per session and parameter set; never modified."""
    key = (tag, kw["max_triangles"], kw.get("rank_mode", 0), mode)
    if key not in _REF:
        _REF[key] = batch_ref.batch(O, problems, kw, mode)
        assert int(_REF[key][0]["tri_total"].max()) <= batch_ref.TRI_CAP
    return _REF[key]


def _pack(problems):
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.uint32)
    return np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems]), off


def _run(reg, pkg, problems, kw, soa=False, **extra):
    """-> (records, mask, offset) of the host form on the packed batch"""
    src, tgt, off = _pack(problems)
    p = pkg.make_params(**kw, layout=pkg.SC_SOA if soa else pkg.SC_AOS, **extra)
    if soa:
        src, tgt = np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)
    recs, mask = reg.register_batch_raw(src, tgt, off, p)
    return recs, mask, off


def _assert_batch(got, exp, what=""):
    recs, mask, off = got
    erecs, emasks = exp
    assert len(recs) == len(erecs), what
    for b in range(len(recs)):
        g, e = recs[b], erecs[b]
        print(what, b, [int(g[f]) for f in FIELDS], "| expected", [int(e[f]) for f in FIELDS])
        assert [int(g[f]) for f in FIELDS] == [int(e[f]) for f in FIELDS], (what, b)
        assert nan_equal_bits(g["Rt"], e["Rt"]), (what, b)
        assert np.array_equal(mask[off[b]: off[b + 1]], emasks[b]), (what, b)


# ---- 1: the mixed batch, both layouts; the cut inside every long list, (almost) no selection, one hypothesis --------------------
@pytest.mark.parametrize("T", [200, 100000, 1])
def test_mixed_batch_equals_the_reference_and_sc_register(pkg, O, reg, T):
    problems = batch_ref.mixed(pkg)
    kw = dict(batch_ref.KW, max_triangles=T)
    exp = _ref(O, "mixed", problems, kw)
    got = _run(reg, pkg, problems, kw)
    _assert_batch(got, exp, f"AoS T={T}")
    _assert_batch(_run(reg, pkg, problems, kw, soa=True), exp, f"SoA T={T}")
    recs, mask, off = got
    for b, (s, t) in enumerate(problems):  # ... and what sc_register returns for the problem alone
        solo = reg.register(s, t, params=pkg.make_params(**kw, flags=SC_FLAG_EXACT_TOTAL))
        st = solo["stats"]
        assert [int(recs[b][f]) for f in FIELDS] == [solo["status"], len(s), st["edges"], st["tri_kept"], st["tri_total"], st["best_rank"],
                                                    st["best_count"]], (T, b)
        assert nan_equal_bits(recs[b]["Rt"], np.concatenate([solo["R"].ravel(), solo["t"]])), (T, b)
        assert np.array_equal(mask[off[b]: off[b + 1]], solo["mask"]), (T, b)
    # the list form returns the same, problem by problem
    if T == 200:
        out = reg.register_batch(problems, params=pkg.make_params(**kw))
        for b, o in enumerate(out):
            assert o["status"] == int(recs[b]["status"]) and o["stats"]["best_count"] == int(recs[b]["best_count"])
            assert np.concatenate([o["R"].ravel(), o["t"]]).tobytes() == recs[b]["Rt"].tobytes()
            assert np.array_equal(o["mask"], mask[off[b]: off[b + 1]])


# ---- 2: equal keys at the cut ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [201, 202, 203])
def test_degree_ranking_ties_at_the_cut(pkg, O, reg, T):
    problems = batch_ref.mixed(pkg)
    kw = dict(batch_ref.KW, max_triangles=T, rank_mode=1)
    _assert_batch(_run(reg, pkg, problems, kw), _ref(O, "mixed", problems, kw), f"degree T={T}")


@pytest.mark.parametrize("T", [1001, 1002, 1003])
def test_every_key_equal(pkg, O, reg, T):
    problems = [batch_ref.exact_scene()]
    kw = dict(batch_ref.KW, max_triangles=T)
    exp = _ref(O, "exact", problems, kw)
    assert (int(exp[0][0]["tri_total"]), int(exp[0][0]["best_rank"]), int(exp[0][0]["best_count"])) == (9880, 0, 40)
    _assert_batch(_run(reg, pkg, problems, kw), exp, f"exact T={T}")
    # ... and the degree ranking, whose keys are all 3 x 39 = 117 here
    kwd = dict(kw, rank_mode=1)
    _assert_batch(_run(reg, pkg, problems, kwd), _ref(O, "exact", problems, kwd), f"exact degree T={T}")


# ---- 3: the truncated score modes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_score_modes(pkg, O, reg, mode):
    problems = batch_ref.mixed(pkg)
    kw = dict(batch_ref.KW, max_triangles=200)
    _assert_batch(_run(reg, pkg, problems, kw, score_mode=mode), _ref(O, "mixed", problems, kw, mode), f"score mode {mode}")


# ---- 4: bad and empty problems between good ones ----------------------------------------------------------------------------------
def test_bad_and_empty_problems_between_good_ones(pkg, O, reg):
    s64, t64 = batch_ref.scene(pkg, 64, .3)
    nan_t = t64.copy(); nan_t[17, 2] = np.nan
    inf_s = s64.copy(); inf_s[63, 0] = np.inf
    problems = [batch_ref.scene(pkg, 128, .3), batch_ref.scene(pkg, 3, 1.0), (s64, nan_t), (inf_s, t64), batch_ref.scene(pkg, 65, .3)]
    kw = dict(batch_ref.KW, max_triangles=200)
    exp = batch_ref.batch(O, problems, kw)
    assert list(exp[0]["status"]) == [SC_OK, SC_ENOHYP, SC_EINVAL, SC_EINVAL, SC_OK]
    for soa in (False, True):
        got = _run(reg, pkg, problems, kw, soa=soa)
        _assert_batch(got, exp, f"soa={soa}")
        for b in (2, 3):  # zeroed as specified
            r = got[0][b]
            assert r["Rt"].tobytes() == batch_ref.IDENT.tobytes() and not got[1][got[2][b]: got[2][b + 1]].any()
            assert [int(r[f]) for f in FIELDS] == [SC_EINVAL, 64, 0, 0, 0, 0, 0]
    for b in (0, 4):  # the good ones equal their solo records
        solo = _run(reg, pkg, [problems[b]], kw)
        assert solo[0][0].tobytes() == got[0][b].tobytes() and np.array_equal(solo[1], got[1][got[2][b]: got[2][b + 1]])


# ---- 5: a record is a function of its own problem and the parameters ---------------------------------------------------------------
def test_independence_of_position_neighbours_and_history(pkg, O, reg):
    problems = batch_ref.mixed(pkg)
    kw = dict(batch_ref.KW, max_triangles=200)
    recs, mask, off = _run(reg, pkg, problems, kw)
    base = [(recs[b].tobytes(), mask[off[b]: off[b + 1]].tobytes()) for b in range(len(problems))]
    _assert_batch((recs, mask, off), _ref(O, "mixed", problems, kw), "base")

    def check(order, what):
        r, m, o = _run(reg, pkg, [problems[b] for b in order], kw)
        for pos, b in enumerate(order):
            assert (r[pos].tobytes(), m[o[pos]: o[pos + 1]].tobytes()) == base[b], (what, b)

    nb = len(problems)
    check(list(range(nb))[::-1], "reversed")
    check([(b + 4) % nb for b in range(nb)], "rotated")
    for b in range(nb):
        check([b], "alone")
    check(list(range(nb)), "again")
    s, t = batch_ref.scene(pkg, 300, .3, seed=99)
    assert reg.register(s, t, params=pkg.make_params(**dict(batch_ref.KW, max_triangles=5000)))["status"] == SC_OK
    check(list(range(nb)), "after an unrelated sc_register")


# ---- 6: more workgroups than compute units ------------------------------------------------------------------------------------------
def test_more_problems_than_compute_units(pkg, O, reg):
    problems = [batch_ref.scene(pkg, 64, .3, seed=8000 + k) for k in range(300)]
    kw = dict(batch_ref.KW, max_triangles=200)
    _assert_batch(_run(reg, pkg, problems, kw), _ref(O, "many64", problems, kw), "300 x 64")


# ---- 7: the device form on a caller's stream ---------------------------------------------------------------------------------------
def test_device_form_on_a_caller_stream(pkg, O, reg):
    import torch
    problems = batch_ref.mixed(pkg)
    kw = dict(batch_ref.KW, max_triangles=200)
    host = _run(reg, pkg, problems, kw)
    src, tgt, off = _pack(problems)
    p = pkg.make_params(**kw)
    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    d_res = torch.zeros(len(problems) * 80, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((int(off[-1]),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    small = batch_ref.scene(pkg, 64, .3)
    reg.set_stream(stream.cuda_stream)
    try:
        reg.register_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_res.data_ptr(), d_mask.data_ptr())
        stream.synchronize()
        recs = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE)
        assert recs.tobytes() == host[0].tobytes() and np.array_equal(d_mask.cpu().numpy(), host[1])
        held = reg.register(*small, params=pkg.make_params(**kw))["stats"]["workspace_bytes"]
        d_res.zero_(); d_mask.fill_(7)
        torch.cuda.synchronize()
        reg.register_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_res.data_ptr(), d_mask.data_ptr())
        stream.synchronize()
        assert d_res.cpu().numpy().tobytes() == host[0].tobytes() and np.array_equal(d_mask.cpu().numpy(), host[1])
        assert reg.register(*small, params=pkg.make_params(**kw))["stats"]["workspace_bytes"] == held  # a second call of the shape: nothing grew
    finally:
        reg.set_stream(None)


# ---- 8: what is refused, and what a batch call leaves --------------------------------------------------------------------------------
def _raw(reg, src, tgt, off, nb, p):
    """the host entry called directly -> (status, sc_last_error)"""
    L = reg._lib
    res = np.zeros(max(nb, 1), batch_ref.RESULT_DTYPE); mask = np.zeros(max(int(off[-1]), 1), np.uint8)
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = L.sc_register_batch(reg._h, src.ctypes.data_as(f32p), tgt.ctypes.data_as(f32p), off.ctypes.data_as(u32p), nb, C.byref(p),
                             res.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.POINTER(C.c_uint8)))
    return rc, L.sc_last_error(reg._h).decode()


def test_refusals_leave_the_context_usable(pkg, O, reg):
    import torch
    s, t = batch_ref.scene(pkg, 128, .3)
    big = np.zeros((513, 3), np.float32)
    kw = dict(batch_ref.KW, max_triangles=200)
    u32 = lambda *a: np.array(a, np.uint32)  # noqa: E731
    cases = {
        "n_b = 2": (s, t, u32(0, 2), 1, pkg.make_params(**kw)),
        "n_b = 513": (big, big, u32(0, 513), 1, pkg.make_params(**kw)),
        "n_problems = 0": (s, t, u32(0), 0, pkg.make_params(**kw)),
        "a decreasing offset": (s, t, u32(0, 64, 60, 128), 3, pkg.make_params(**kw)),
        "SC_FLAG_REFINE": (s, t, u32(0, 128), 1, pkg.make_params(**kw, flags=SC_FLAG_REFINE)),
        "SC_FLAG_TIMING": (s, t, u32(0, 128), 1, pkg.make_params(**kw, flags=SC_FLAG_TIMING)),
        "shard_world = 2": (s, t, u32(0, 128), 1, pkg.make_params(**kw, shard_world=2)),
    }
    good = reg.register(s, t, params=pkg.make_params(**kw))
    for what, (a, b, off, nb, p) in cases.items():
        rc, err = _raw(reg, a, b, off, nb, p)
        print(what, rc, err)
        assert rc == SC_EINVAL and "sc_register_batch" in err, what
        again = reg.register(s, t, params=pkg.make_params(**kw))  # the context stays usable
        assert again["status"] == SC_OK and np.array_equal(again["mask"], good["mask"]) and again["R"].tobytes() == good["R"].tobytes(), what
    # a call outstanding on the context
    d_s, d_t = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
    d_rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_m = torch.zeros(128, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = pkg.make_params(**kw)
    reg.register_device_async(d_s.data_ptr(), d_t.data_ptr(), 128, p, d_rt.data_ptr(), d_m.data_ptr())
    rc, err = _raw(reg, s, t, u32(0, 128), 1, p)
    assert rc == SC_EINVAL and "outstanding" in err
    rc, _ = reg.wait()
    assert rc == SC_OK and np.array_equal(d_m.cpu().numpy(), good["mask"])
    # a batch call ends the frame and leaves none
    assert reg.register(s, t, params=p)["status"] == SC_OK
    recs, _ = reg.register_batch_raw(s, t, u32(0, 128), p)
    assert recs[0]["status"] == SC_OK and recs[0]["best_count"] == good["stats"]["best_count"]
    for call in (reg.peel, reg.polish):
        with pytest.raises(pkg.SacCotError) as e:
            call()
        assert e.value.status == SC_EINVAL


# ---- 9: a host-array entry that the workspace cap refuses --------------------------------------------------------------------------
def _assert_records(recs, erecs, what):
    for b, (g, e) in enumerate(zip(recs, erecs)):
        assert [int(g[f]) for f in FIELDS] == [int(e[f]) for f in FIELDS], (what, b)
        assert nan_equal_bits(g["Rt"], e["Rt"]), (what, b)


def _assert_slots(got, exp, slot, what):
    """(records, corr, d2, count, mask) of a features entry against [dict(corr, d2, n, flag, rec, mask)], problem b's slot at slot[b]"""
    recs, corr, d2, count, mask = got
    assert len(recs) == len(exp), what
    _assert_records(recs, [e["rec"] for e in exp], what)
    for b, e in enumerate(exp):
        lo, n = int(slot[b]), e["n"]
        assert count[b].tolist() == [n, e["flag"]], (what, b)
        assert np.array_equal(corr[lo: lo + n], e["corr"]) and d2[lo: lo + n].tobytes() == e["d2"].tobytes(), (what, b)
        assert np.array_equal(mask[lo: lo + len(e["mask"])], e["mask"]), (what, b)


def test_a_capped_workspace_refuses_before_anything_is_enqueued(pkg, O):
    """max_workspace = 1: the first buffer an entry asks for is SC_ENOMEM on a fresh context and on a used one — host arithmetic,
    made before the first copy or launch.  The same call under the default cap on the same context then equals the reference.  (The
    host forms' device copies are one pool: the last entry finds every buffer it needs on the used context, so its refusal is shown on
    a fresh one, and on the used one it runs under the same cap.)"""
    import torch
    reg = pkg.Registrar(0)
    try:
        problems = [batch_ref.scene(pkg, 64, .3), batch_ref.scene(pkg, 64, .3, seed=8000)]
        kw = dict(batch_ref.KW, max_triangles=200)
        src, tgt, off = _pack(problems)
        p, tight = pkg.make_params(**kw), pkg.make_params(**kw, max_workspace=1)
        q = pkg.make_polish_params(candidates=1, max_iter=16)
        exp = batch_ref.batch(O, problems, kw)
        mkw = dict(knn=1, mutual=True)
        mp = pkg.api.make_match_params(33, **mkw)
        scenes = M.feature_scenes()[:2]  # (the two smallest)
        so, to = reg._offsets([len(s[1]) for s in scenes]), reg._offsets([len(s[3]) for s in scenes])
        packed = [np.concatenate([s[k] for s in scenes]) for k in range(4)]
        tab = P.table()
        pairs = np.array([(P.R1, P.R2), (P.R2, P.R1)], np.uint32)  # (the two smallest sets)

        def refused(call, what):
            with pytest.raises(pkg.SacCotError) as e:
                call()
            print(what, e.value)
            assert e.value.status == SC_ENOMEM, what

        # a device form first, on the fresh context: its outputs keep what they held
        d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
        d_res = torch.full((len(problems) * 80,), 0xAB, dtype=torch.uint8, device="cuda")
        d_mask = torch.full((int(off[-1]),), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        run = lambda a: reg.register_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, a, d_res.data_ptr(), d_mask.data_ptr())  # noqa: E731
        refused(lambda: run(tight), "sc_register_batch_device")
        torch.cuda.synchronize()
        assert bool((d_res == 0xAB).all()) and bool((d_mask == 7).all())
        run(p)
        torch.cuda.synchronize()
        _assert_batch((np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE), d_mask.cpu().numpy(), off), exp,
                      "sc_register_batch_device")

        # the host forms, each refused by the first buffer of its own that is not there yet, and then run
        run = lambda a: reg.register_batch_raw(src, tgt, off, a)  # noqa: E731
        refused(lambda: run(tight), "sc_register_batch")
        recs, mask = run(p)
        _assert_batch((recs, mask, off), exp, "sc_register_batch")

        run = lambda a: reg.polish_batch_raw(src, tgt, off, a, q, recs)  # noqa: E731
        refused(lambda: run(tight), "sc_polish_batch")
        pol, pmask = run(p)
        epol, epmasks = PB.batch(O, problems, exp[0], kw["tau"], 0, 16)
        for b in range(len(problems)):
            assert [int(pol[b][f]) for f in PB.FIELDS] == [int(epol[b][f]) for f in PB.FIELDS], b
            assert nan_equal_bits(pol[b]["Rt"], epol[b]["Rt"]) and np.array_equal(pmask[off[b]: off[b + 1]], epmasks[b]), b

        run = lambda a: reg.register_instances_batch_raw(src, tgt, off, a, 4, 4)  # noqa: E731
        refused(lambda: run(tight), "sc_register_instances_batch")
        irecs, label, nfound = run(p)
        erecs, elabels, efound = IR.batch(O, problems, kw, 0, 4, 4)
        assert irecs.shape == erecs.shape and nfound.tolist() == efound.tolist()
        for b in range(len(problems)):
            _assert_records(irecs[:, b], erecs[:, b], ("sc_register_instances_batch", b))
            assert np.array_equal(label[off[b]: off[b + 1]], elabels[b]), b

        run = lambda a: reg.register_pairs_features(tab["pts"], tab["feat"], tab["set_off"], pairs, mp, a)  # noqa: E731
        refused(lambda: run(pkg.make_params(**P.KW, max_workspace=1)), "sc_register_pairs_features")
        got = run(pkg.make_params(**P.KW))
        _assert_slots(got[:5], P.features(O, tab, pairs, mkw, P.KW), got[5], "sc_register_pairs_features")

        # the packed form of the same family: refused on a context of its own.  On this one nothing of its own is missing — the match's
        # buffers are the pairs form's, and the nine slots of the host forms' pool were warmed by the entries above (every array here is
        # below the 64 KiB a slot holds at least) — and a call that allocates nothing is refused by no cap: it equals the reference
        run = lambda a, r=reg: r.register_batch_features_raw(packed[0], packed[1], so, packed[2], packed[3], to, mp, a)  # noqa: E731
        fresh = pkg.Registrar(0)
        try:
            refused(lambda: run(pkg.make_params(**M.KW, max_workspace=1), fresh), "sc_register_batch_features")
        finally:
            fresh.close()
        efeat = [M.features_one(O, s[0], s[1], s[2], s[3], mkw, M.KW) for s in scenes]
        slot = so.astype(np.int64) * int(mp.knn)
        _assert_slots(run(pkg.make_params(**M.KW, max_workspace=1)), efeat, slot, "sc_register_batch_features, nothing to allocate")
        _assert_slots(run(pkg.make_params(**M.KW)), efeat, slot, "sc_register_batch_features")
    finally:
        reg.close()
