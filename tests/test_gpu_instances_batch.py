"""GPU: several rigid motions per batch problem (include/saccot.h, sc_register_instances_batch*).

The expected value of every case is tests/instances_batch_ref.py — per problem plane 0 through the CPU restatement's whole path,
the motions composed from its stage functions — and everything is compared bit for bit: every field of every record of every
plane, every label, every nfound.  No tolerances.  The scenes are checked on the CPU by tests/test_instances_batch_abi.py (at most
batch_ref.TRI_CAP triangles a problem, so no workgroup runs long).
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref
import instances_batch_ref as IR
import match_batch_ref as M
from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
SC_FLAG_TIMING, SC_FLAG_EXACT_TOTAL, SC_FLAG_REFINE = 1, 2, 8
FIELDS = ("status", "n", "edges", "tri_kept", "tri_total", "best_rank", "best_count")

_REF = {}


def _ref(O, tag, problems, kw, mode=0, max_instances=4, min_score=4):
    """The reference of a set of problems, once per session and parameter set; never modified."""
    key = (tag, kw["max_triangles"], kw.get("rank_mode", 0), mode, max_instances, min_score)
    if key not in _REF:
        _REF[key] = IR.batch(O, problems, kw, mode, max_instances, min_score)
        assert int(_REF[key][0]["tri_total"].max()) <= batch_ref.TRI_CAP
    return _REF[key]


def _pack(problems):
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.uint32)
    return np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems]), off


def _run(reg, pkg, problems, kw, max_instances=4, min_score=4, soa=False, **extra):
    """-> (records (max_instances, B), label, nfound, offset) of the host form on the packed batch"""
    src, tgt, off = _pack(problems)
    p = pkg.make_params(**kw, layout=pkg.SC_SOA if soa else pkg.SC_AOS, **extra)
    if soa:
        src, tgt = np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)
    recs, label, nfound = reg.register_instances_batch_raw(src, tgt, off, p, max_instances, min_score)
    return recs, label, nfound, off


def _assert_batch(got, exp, what=""):
    recs, label, nfound, off = got
    erecs, elabels, efound = exp
    assert recs.shape == erecs.shape, what
    for b in range(recs.shape[1]):
        print(what, b, "found", int(nfound[b]), [int(x) for x in recs[:, b]["best_count"]], [int(x) for x in recs[:, b]["best_rank"]],
              "| expected", int(efound[b]), [int(x) for x in erecs[:, b]["best_count"]], [int(x) for x in erecs[:, b]["best_rank"]])
        assert int(nfound[b]) == int(efound[b]), (what, b)
        for k in range(recs.shape[0]):
            g, e = recs[k, b], erecs[k, b]
            assert [int(g[f]) for f in FIELDS] == [int(e[f]) for f in FIELDS], (what, b, k)
            assert nan_equal_bits(g["Rt"], e["Rt"]), (what, b, k)
        assert np.array_equal(label[off[b]: off[b + 1]], elabels[b]), (what, b)


def _bytes(got, b):
    recs, label, nfound, off = got
    return recs[:, b].tobytes(), label[off[b]: off[b + 1]].tobytes(), int(nfound[b])


# ---- 1: the mixed batch, both layouts, either ranking, every score mode; with and without a short list ---------------------------
@pytest.mark.parametrize("T", [2000, 50])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("rank_mode", [0, 1])
def test_mixed_batch_equals_the_reference(pkg, O, reg, rank_mode, mode, T):
    problems = IR.scenes(pkg)
    kw = dict(IR.KW, max_triangles=T, rank_mode=rank_mode)
    min_score = 4 if mode == 0 else 4 * 256  # (a truncated score is 1024 per perfect inlier)
    exp = _ref(O, "scenes", problems, kw, mode, 4, min_score)
    what = f"rank {rank_mode} mode {mode} T={T}"
    _assert_batch(_run(reg, pkg, problems, kw, 4, min_score, score_mode=mode), exp, "AoS " + what)
    _assert_batch(_run(reg, pkg, problems, kw, 4, min_score, soa=True, score_mode=mode), exp, "SoA " + what)


# ---- 2: the library against itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2000, 50])
def test_every_problem_equals_sc_register_instances_on_it_alone(pkg, reg, T):
    problems = IR.scenes(pkg)
    kw = dict(IR.KW, max_triangles=T)
    recs, label, nfound, off = _run(reg, pkg, problems, kw, 4, 4)
    for b, (s, t) in enumerate(problems):
        solo = reg.register_instances(s, t, max_instances=4, min_score=4, params=pkg.make_params(**kw, flags=SC_FLAG_EXACT_TOTAL))
        k = len(solo["score"])
        print(T, b, k, solo["score"], int(nfound[b]))
        assert k == int(nfound[b]) and solo["status"] == int(recs[0, b]["status"]), (T, b)
        assert nan_equal_bits(solo["Rt"], recs[:k, b]["Rt"]) and np.array_equal(solo["score"], recs[:k, b]["best_count"]), (T, b)
        assert np.array_equal(solo["label"], label[off[b]: off[b + 1]]), (T, b)
        st = solo["stats"]
        assert [int(recs[0, b][f]) for f in FIELDS[1:]] == [len(s), st["edges"], st["tri_kept"], st["tri_total"], st["best_rank"],
                                                            st["best_count"]], (T, b)
    out = reg.register_instances_batch(problems, max_instances=4, min_score=4, params=pkg.make_params(**kw))  # the list form
    for b, o in enumerate(out):
        k = int(nfound[b])
        assert o["status"] == int(recs[0, b]["status"]) and o["Rt"].tobytes() == recs[:k, b]["Rt"].tobytes()
        assert np.array_equal(o["score"], recs[:k, b]["best_count"]) and np.array_equal(o["label"], label[off[b]: off[b + 1]])


# ---- 3: plane 0 is sc_register_batch's record, whatever min_score is --------------------------------------------------------------
def test_plane_0_is_the_batch_record(pkg, reg):
    problems = IR.scenes(pkg)
    kw = dict(IR.KW, max_triangles=200)
    src, tgt, off = _pack(problems)
    brecs, bmask = reg.register_batch_raw(src, tgt, off, pkg.make_params(**kw))
    for min_score in (0, 4, 10 ** 6):
        recs, label, nfound, _ = _run(reg, pkg, problems, kw, 4, min_score)
        assert recs[0].tobytes() == brecs.tobytes(), min_score
    assert not nfound.any() and (label == -1).all()  # min_score 10^6: nothing is found
    assert (recs[1:]["status"] == SC_ENOHYP).all() and not recs[1:]["best_count"].any()
    recs, label, nfound, _ = _run(reg, pkg, problems, kw, 1, 0)
    assert recs.shape[0] == 1 and recs[0].tobytes() == brecs.tobytes()
    assert np.array_equal(label == 0, bmask.astype(bool)) and set(np.unique(label)) == {-1, 0}
    assert np.array_equal(nfound, (brecs["status"] == SC_OK).astype(np.uint32))


# ---- 4: every key equal: the cut among ties decides the selection and the rank in every round -------------------------------------
@pytest.mark.parametrize("T", [1, 7, 100000])
def test_every_key_equal(pkg, O, reg, T):
    problems = [batch_ref.exact_scene()]
    for rank_mode in (0, 1):
        kw = dict(IR.KW, max_triangles=T, rank_mode=rank_mode)
        exp = _ref(O, "exact", problems, kw, 0, 4, 0)
        assert int(exp[0][0, 0]["tri_total"]) == 9880 and int(exp[0][0, 0]["tri_kept"]) == min(T, 9880)
        _assert_batch(_run(reg, pkg, problems, kw, 4, 0), exp, f"exact T={T} rank {rank_mode}")


# ---- 5: rounds until nothing scores ---------------------------------------------------------------------------------------------------
def test_rounds_until_nothing_scores(pkg, O, reg):
    problems = [IR.scene(pkg, 65, .5)]
    kw = dict(IR.KW, max_triangles=2000)
    exp = _ref(O, "n65", problems, kw, 0, 16, 0)
    got = _run(reg, pkg, problems, kw, 16, 0)
    _assert_batch(got, exp, "16 planes")
    recs, label, nfound, _ = got
    k = int(nfound[0])
    print("found", k, [int(x) for x in recs[:, 0]["best_count"]])
    assert 2 <= k < 16
    assert (recs[k:, 0]["status"] == SC_ENOHYP).all() and all(r["Rt"].tobytes() == batch_ref.IDENT.tobytes() for r in recs[k:, 0])
    assert all(recs[j, 0][f] == recs[0, 0][f] for j in range(16) for f in ("n", "edges", "tri_kept", "tri_total"))
    # a correspondence has ONE label, and a motion's score is what it claimed (inlier count)
    assert [int((label == j).sum()) for j in range(k)] == [int(x) for x in recs[:k, 0]["best_count"]]
    assert label.min() >= -1 and label.max() == k - 1


# ---- 6: a problem's outputs are a function of the problem and the parameters --------------------------------------------------------
def test_independence_of_position_neighbours_and_history(pkg, reg):
    problems = IR.scenes(pkg)
    kw = dict(IR.KW, max_triangles=50)
    got = _run(reg, pkg, problems, kw, 4, 4)
    base = [_bytes(got, b) for b in range(len(problems))]

    def check(order, what):
        g = _run(reg, pkg, [problems[b] for b in order], kw, 4, 4)
        for pos, b in enumerate(order):
            assert _bytes(g, pos) == base[b], (what, b)

    nb = len(problems)
    check(list(range(nb))[::-1], "reversed")
    check([(b + 3) % nb for b in range(nb)], "rotated")
    for b in range(nb):
        check([b], "alone")
    s, t = batch_ref.scene(pkg, 300, .3, seed=99)
    assert reg.register(s, t, params=pkg.make_params(**dict(IR.KW, max_triangles=5000)))["status"] == SC_OK
    check(list(range(nb)), "after an unrelated sc_register")
    reg.register_batch_raw(*_pack(problems[2:5]), pkg.make_params(**kw))
    check(list(range(nb)), "after an sc_register_batch")


# ---- 7: bad and empty problems between good ones -------------------------------------------------------------------------------------
def test_bad_and_empty_problems_between_good_ones(pkg, O, reg):
    s64, t64 = IR.scene(pkg, 64, .5)
    nan_t = t64.copy(); nan_t[17, 2] = np.nan
    zero = np.zeros((40, 3), np.float32)  # every pair shorter than min_len: no edge
    problems = [IR.scene(pkg, 128, .5), IR.scene(pkg, 3, 1.0), (s64, nan_t), (zero, zero), IR.scene(pkg, 65, .5)]
    kw = dict(IR.KW, max_triangles=2000)
    exp = IR.batch(O, problems, kw, 0, 4, 4)
    assert list(exp[0][0]["status"]) == [SC_OK, SC_ENOHYP, SC_EINVAL, SC_ENOHYP, SC_OK] and list(exp[2]) == [2, 0, 0, 0, 2]
    assert exp[0][0, 3]["edges"] == 0
    for soa in (False, True):
        got = _run(reg, pkg, problems, kw, 4, 4, soa=soa)
        _assert_batch(got, exp, f"soa={soa}")
        recs, label, nfound, off = got
        assert (recs[:, 2]["status"] == SC_EINVAL).all() and (recs[:, 2]["n"] == 64).all() and not recs[:, 2]["edges"].any()
        for b in (1, 2, 3):
            assert (label[off[b]: off[b + 1]] == -1).all()
    for b in (0, 4):  # the good ones equal their solo outputs
        assert _bytes(_run(reg, pkg, [problems[b]], kw, 4, 4), 0) == _bytes(got, b)


# ---- 8: the slot form equals the plain form on the gathered correspondences ----------------------------------------------------------
@pytest.mark.parametrize("knn", [1, 2])
def test_features_form_equals_the_plain_form_on_the_gathered_correspondences(pkg, reg, knn):
    import torch
    scenes = [list(s[:4]) for s in M.feature_scenes()]
    scenes[4][1] = scenes[4][1].copy(); scenes[4][1][0, 0] = np.inf  # a flagged problem
    scenes[0] = [scenes[0][0][:1], scenes[0][1][:1], scenes[0][2], scenes[0][3]]  # one source keypoint: fewer than three matches
    mp = pkg.api.make_match_params(33, knn=knn, mutual=(knn == 1))
    kw = dict(IR.KW, max_triangles=50)
    p = pkg.make_params(**kw)
    so = reg._offsets([len(s[1]) for s in scenes]); to = reg._offsets([len(s[3]) for s in scenes])
    src, fsrc = np.concatenate([s[0] for s in scenes]), np.concatenate([s[1] for s in scenes])
    tgt, ftgt = np.concatenate([s[2] for s in scenes]), np.concatenate([s[3] for s in scenes])
    nb, slots, K = len(scenes), int(so[-1]) * knn, 3
    h_res, h_corr, h_d2, h_count, h_mask = reg.register_batch_features_raw(src, fsrc, so, tgt, ftgt, to, mp, p)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = [dev(a) for a in (src, fsrc, tgt, ftgt)]
    d_res = torch.zeros(K * nb * 80, dtype=torch.uint8, device="cuda")
    d_corr = torch.zeros((slots, 2), dtype=torch.int32, device="cuda"); d_d2 = torch.zeros(slots, dtype=torch.float32, device="cuda")
    d_count = torch.zeros((nb, 2), dtype=torch.int32, device="cuda")
    d_label = torch.full((slots,), 77, dtype=torch.int32, device="cuda"); d_nfound = torch.full((nb,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    reg.register_instances_batch_features_device(d[0].data_ptr(), d[1].data_ptr(), so, d[2].data_ptr(), d[3].data_ptr(), to, mp, p, K, 4,
                                                 d_res.data_ptr(), d_corr.data_ptr(), d_d2.data_ptr(), d_count.data_ptr(),
                                                 d_label.data_ptr(), d_nfound.data_ptr())
    torch.cuda.synchronize()
    recs = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE).reshape(K, nb)
    count, corr = d_count.cpu().numpy().astype(np.uint32), d_corr.cpu().numpy()
    label, nfound = d_label.cpu().numpy(), d_nfound.cpu().numpy()
    assert np.array_equal(count, h_count) and recs[0].tobytes() == h_res.tobytes()  # the match, and plane 0
    assert count[4, 1] == 1 and count[0, 0] < 3 and (count[:, 0] >= 3).sum() >= 5
    good = [b for b in range(nb) if count[b, 1] == 0 and count[b, 0] >= 3]
    gathered = []
    for b in good:
        lo, n = int(so[b]) * knn, int(count[b, 0])
        c = corr[lo: lo + n]
        assert np.array_equal(c, h_corr[lo: lo + n])
        gathered.append((scenes[b][0][c[:, 0]], scenes[b][2][c[:, 1]]))
    precs, plabel, pfound, poff = _run(reg, pkg, gathered, kw, K, 4)
    for pos, b in enumerate(good):
        lo, n = int(so[b]) * knn, int(count[b, 0])
        print(knn, b, n, int(nfound[b]), [int(x) for x in recs[:, b]["best_count"]])
        assert recs[:, b].tobytes() == precs[:, pos].tobytes() and int(nfound[b]) == int(pfound[pos]), (knn, b)
        assert np.array_equal(label[lo: lo + n], plabel[poff[pos]: poff[pos + 1]]), (knn, b)
    assert nfound[good].max() >= 1
    for b in set(range(nb)) - set(good):  # flagged: SC_EINVAL, n = 0; short: SC_ENOHYP, n = n_b, its labels -1 — in every plane
        flagged = count[b, 1] != 0
        lo, n = int(so[b]) * knn, int(count[b, 0])
        assert nfound[b] == 0 and (recs[:, b]["status"] == (SC_EINVAL if flagged else SC_ENOHYP)).all(), b
        assert (recs[:, b]["n"] == (0 if flagged else n)).all() and not recs[:, b]["edges"].any(), b
        assert all(r["Rt"].tobytes() == batch_ref.IDENT.tobytes() for r in recs[:, b]), b
        assert (label[lo: lo + n] == -1).all(), b


# ---- 9: the device form; refusals leave the context usable; the workspace appears with the first call ---------------------------------
def _raw(reg, src, tgt, off, nb, p, max_instances=4):
    """the host entry called directly -> (status, sc_last_error)"""
    L = reg._lib
    res = np.zeros(16 * max(nb, 1), batch_ref.RESULT_DTYPE); label = np.zeros(max(int(off[-1]), 1), np.int32)
    nfound = np.zeros(max(nb, 1), np.uint32)
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = L.sc_register_instances_batch(reg._h, src.ctypes.data_as(f32p), tgt.ctypes.data_as(f32p), off.ctypes.data_as(u32p), nb, C.byref(p),
                                       max_instances, 4, res.ctypes.data_as(C.c_void_p), label.ctypes.data_as(C.POINTER(C.c_int32)),
                                       nfound.ctypes.data_as(u32p))
    return rc, L.sc_last_error(reg._h).decode()


def test_refusals_and_workspace(pkg):
    import torch
    reg = pkg.Registrar(0)  # a context of its own: what it holds is this test's
    try:
        s, t = IR.scene(pkg, 128, .5)
        big = np.zeros((513, 3), np.float32)
        kw = dict(IR.KW, max_triangles=2000)
        p = pkg.make_params(**kw)
        u32 = lambda *a: np.array(a, np.uint32)  # noqa: E731
        good = reg.register(s, t, params=p)
        held = good["stats"]["workspace_bytes"]
        cases = {
            "max_instances = 0": (s, t, u32(0, 128), 1, p, 0, "max_instances"),
            "max_instances = 17": (s, t, u32(0, 128), 1, p, 17, "max_instances"),
            "n_b = 2": (s, t, u32(0, 2), 1, p, 4, "fewer than 3"),
            "n_b = 513": (big, big, u32(0, 513), 1, p, 4, "SC_BATCH_MAX_N"),
            "n_problems = 0": (s, t, u32(0), 0, p, 4, "n_problems"),
            "a decreasing offset": (s, t, u32(0, 64, 60, 128), 3, p, 4, "decrease"),
            "SC_FLAG_REFINE": (s, t, u32(0, 128), 1, pkg.make_params(**kw, flags=SC_FLAG_REFINE), 4, "accepted"),
            "SC_FLAG_TIMING": (s, t, u32(0, 128), 1, pkg.make_params(**kw, flags=SC_FLAG_TIMING), 4, "accepted"),
            "shard_world = 2": (s, t, u32(0, 128), 1, pkg.make_params(**kw, shard_world=2), 4, "shard_world"),
        }
        for what, (a, b, off, nb, q, k, word) in cases.items():
            rc, err = _raw(reg, a, b, off, nb, q, k)
            print(what, rc, err)
            assert rc == SC_EINVAL and "sc_register_instances_batch" in err and word in err, what
            again = reg.register(s, t, params=p)  # the context stays usable, and nothing was allocated
            assert again["status"] == SC_OK and np.array_equal(again["mask"], good["mask"]) and again["R"].tobytes() == good["R"].tobytes(), what
            assert again["stats"]["workspace_bytes"] == held, what
        # the first call allocates (the offsets, the host form's copies), a second of the shape does not
        host = reg.register_instances_batch_raw(s, t, u32(0, 128), p, 4, 4)
        first = reg.register(s, t, params=p)["stats"]["workspace_bytes"]
        assert first > held
        assert _bytes(reg.register_instances_batch_raw(s, t, u32(0, 128), p, 4, 4) + (u32(0, 128),), 0) == _bytes(host + (u32(0, 128),), 0)
        assert reg.register(s, t, params=p)["stats"]["workspace_bytes"] == first
        # the device form on a caller's stream: the same bytes
        d_s, d_t = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
        d_res = torch.zeros(4 * 80, dtype=torch.uint8, device="cuda")
        d_label = torch.full((128,), 77, dtype=torch.int32, device="cuda"); d_nf = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        reg.set_stream(stream.cuda_stream)
        try:
            reg.register_instances_batch_device(d_s.data_ptr(), d_t.data_ptr(), u32(0, 128), p, 4, 4, d_res.data_ptr(), d_label.data_ptr(),
                                                d_nf.data_ptr())
            stream.synchronize()
        finally:
            reg.set_stream(None)
        assert d_res.cpu().numpy().tobytes() == host[0].tobytes() and np.array_equal(d_label.cpu().numpy(), host[1])
        assert int(d_nf.cpu().numpy()[0]) == int(host[2][0]) == 2
        # a call outstanding on the context
        d_rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_m = torch.zeros(128, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        reg.register_device_async(d_s.data_ptr(), d_t.data_ptr(), 128, p, d_rt.data_ptr(), d_m.data_ptr())
        rc, err = _raw(reg, s, t, u32(0, 128), 1, p)
        assert rc == SC_EINVAL and "outstanding" in err
        rc, _ = reg.wait()
        assert rc == SC_OK and np.array_equal(d_m.cpu().numpy(), good["mask"])
        # the call ends the frame and leaves none
        assert reg.register(s, t, params=p)["status"] == SC_OK
        reg.register_instances_batch_raw(s, t, u32(0, 128), p, 4, 4)
        for call in (reg.peel, reg.polish):
            with pytest.raises(pkg.SacCotError) as e:
                call()
            assert e.value.status == SC_EINVAL
    finally:
        reg.close()
