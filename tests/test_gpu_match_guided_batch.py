"""GPU: pose-gated matching for a batch of problems (include/saccot.h, sc_match_guided_batch / sc_match_guided_batch_device /
sc_register_guided_batch_features_device).

Every comparison is bit for bit against the numpy restatement (tests/match_guided_batch_ref.py): the slots, the bits of the squared
distances and of the gate residuals, the count pairs — and the outputs are filled before every device call, so that a write outside
[slot, slot + n_b) shows.  tests/test_match_guided_batch_abi.py checks, on the CPU, that the restatement with an open gate is
match_batch_ref and that the shared batch holds what it is used for here.
"""
import numpy as np
import pytest

import match_batch_ref as M
import match_guided_batch_ref as GB
import match_guided_ref as MG
from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
FIELDS = ("status", "n", "edges", "tri_kept", "tri_total", "best_rank", "best_count")


@pytest.fixture(scope="module")
def greg(pkg):
    r = pkg.Registrar(0)
    yield r
    r.close()


# ---- 1: the mixed batch: descriptor lengths x modes x layouts x gates ------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 33])
def test_the_batch_equals_the_restatement(pkg, greg, D):
    batch = GB.shared_batch(D)
    for layout in (0, pkg.SC_SOA):
        for kw in MG.MODES:
            for gate in (MG.GATE, MG.GATE_NOTHING):
                exp = GB.match_batch(batch, gate, **kw)
                got = GB.run_device(pkg, greg, batch, gate, layout=layout, **kw)
                GB.same(got, exp, (D, layout, kw, gate))
                if gate == MG.GATE_NOTHING:
                    assert not got[3].any()  # all counts 0, and that is no flag
                else:  # the gate bites in the large problems and keeps something; the hostile pose admits nothing, unflagged
                    if len(kw) == 1:
                        assert 0 < got[3][4, 0] < 300 * kw["knn"] and got[3][GB.SKIP_AT, 0] > 100
                    assert got[3][GB.HOSTILE_AT].tolist() == [0, 0] and not got[3][:, 1].any()


def test_an_open_gate_equals_the_plain_batch_match(pkg, greg):
    for D in (1, 33):
        batch = GB.mixed_batch(D)
        so, to = batch.offsets()
        _, fs, _, ft = batch.packed()
        for kw in MG.MODES:
            got = GB.run_device(pkg, greg, batch, MG.GATE_ALL, **kw)
            GB.same(got, GB.match_batch(batch, MG.GATE_ALL, **kw), ("open gate", D, kw))
            corr, d2, count = greg.match_batch_raw(fs, so, ft, to, pkg.api.make_match_params(D, **kw))
            assert np.array_equal(count, got[3]) and count[:, 0].all(), (D, kw)
            knn = kw.get("knn", 1)
            for b in range(len(batch)):  # the bytes of every slot equal sc_match_batch's
                lo, n = int(so[b]) * knn, int(count[b, 0])
                assert corr[lo: lo + n].tobytes() == got[0][lo: lo + n].tobytes() and d2[lo: lo + n].tobytes() == got[1][lo: lo + n].tobytes(), (D, kw, b)


def test_one_run_at_dim_352(pkg, greg):
    batch = GB.mixed_batch(352)
    GB.same(GB.run_device(pkg, greg, batch, MG.GATE, layout=pkg.SC_SOA, knn=1, mutual=True), GB.match_batch(batch, MG.GATE, knn=1, mutual=True), "D = 352")


# ---- 2: the skip path and the flag -------------------------------------------------------------------------------------------------
def test_skipped_tiles_and_the_non_finite_flag(pkg, greg):
    """the cluster problem between two ordinary ones; a non-finite value in descriptors and points that only skipped tiles would
    stage, and in its pose: its count pair is (0, 1), the neighbours' bytes are what they were, the host form returns SC_OK"""
    shared = GB.shared_batch(33)
    batch = GB.Batch([shared.scenes[2], shared.scenes[GB.SKIP_AT], shared.scenes[3]])
    so, _ = batch.offsets()
    lo, hi = int(so[1]), int(so[2])
    clean = {}
    for kw in (dict(knn=1), dict(knn=1, mutual=True)):
        key = tuple(sorted(kw.items()))
        clean[key] = GB.run_device(pkg, greg, batch, MG.GATE, **kw)
        GB.same(clean[key], GB.match_batch(batch, MG.GATE, **kw), ("clean", kw))
        assert clean[key][3][1, 0] > 40
    cases = []
    for val in (np.nan, np.inf):  # rows 256 .. 383 and columns 128 .. 191 are staged by no tile that is computed
        cases += [("fsrc", (300, 7), val), ("ftgt", (150, 32), val), ("src_pts", (300, 1), val), ("tgt_pts", (150, 2), val)]
    cases += [("fsrc", (383, 32), -np.inf), ("tgt_pts", (191, 0), np.nan), ("Rt", (0,), np.nan), ("Rt", (5,), np.inf), ("Rt", (11,), -np.inf)]
    for which, pos, val in cases:
        arr = np.array(getattr(batch.scenes[1], which)); arr[pos] = val
        bad = GB.with_scene(batch, 1, **{which: arr})
        for layout, kw in ((0, dict(knn=1)), (pkg.SC_SOA, dict(knn=1, mutual=True))):
            got = GB.run_device(pkg, greg, bad, MG.GATE, layout=layout, **kw)
            ref = clean[tuple(sorted(kw.items()))]
            print(which, pos, val, kw, got[3].tolist())
            assert got[3][1].tolist() == [0, 1], (which, pos, val, kw)
            assert np.array_equal(np.delete(got[3], 1, 0), np.delete(ref[3], 1, 0)), (which, pos, val, kw)
            for a in (0, 1, 2):  # the neighbours' slots, bit for bit; the flagged problem's slot is not written
                assert np.delete(got[a], np.s_[lo:hi], 0).tobytes() == np.delete(ref[a], np.s_[lo:hi], 0).tobytes(), (which, pos, val, kw, a)
            assert (got[0][lo:hi] == GB.FILL_I).all() and (got[1][lo:hi] == np.float32(GB.FILL_F)).all()
        if which in ("fsrc", "tgt_pts", "Rt") and val is not np.inf:
            host = GB.run_host(greg, bad, MG.GATE, knn=1)  # the call itself is SC_OK: no exception
            GB.same(host, GB.match_batch(bad, MG.GATE, knn=1), ("host form", which, pos))
    GB.same(GB.run_device(pkg, greg, batch, MG.GATE, knn=2), GB.match_batch(batch, MG.GATE, knn=2), "the context is usable afterwards")


# ---- 3: a problem's outputs are a function of the problem -------------------------------------------------------------------------
def test_independence_of_position_neighbours_and_history(pkg, greg):
    shared = GB.shared_batch(33)
    me = shared.scenes[3]  # (130, 129): three row tiles, three column tiles
    alone = GB.Batch([me])
    order = [4, 0, GB.SKIP_AT, None, 2, GB.HOSTILE_AT, 1]
    middle = GB.Batch([me if b is None else shared.scenes[b] for b in order])
    at = order.index(None)
    so, _ = middle.offsets()
    for kw in (dict(knn=1), dict(knn=4), dict(knn=1, mutual=True), dict(knn=1, ratio=0.8)):
        knn = kw.get("knn", 1)
        a = GB.run_device(pkg, greg, alone, MG.GATE, **kw)
        m = GB.run_device(pkg, greg, middle, MG.GATE, **kw)
        GB.same(m, GB.match_batch(middle, MG.GATE, **kw), ("in the middle of 7", kw))
        fresh = pkg.Registrar(0)
        try:
            f = GB.run_device(pkg, fresh, alone, MG.GATE, **kw)
        finally:
            fresh.close()
        lo, hi = int(so[at]) * knn, int(so[at + 1]) * knn
        assert a[3][0, 0] > 0 and a[3][0].tolist() == m[3][at].tolist() == f[3][0].tolist(), kw
        for k in (0, 1, 2):
            assert a[k].tobytes() == m[k][lo:hi].tobytes() == f[k].tobytes(), (kw, k)


# ---- 4: device and host forms, with and without g2 ----------------------------------------------------------------------------------
def test_device_and_host_forms_agree(pkg, greg):
    batch = GB.shared_batch(33)
    for kw in (dict(knn=3), dict(knn=1, mutual=True, ratio=0.9)):
        exp = GB.match_batch(batch, MG.GATE, **kw)
        for layout in (0, pkg.SC_SOA):
            for want_g2 in (True, False):
                dev = GB.run_device(pkg, greg, batch, MG.GATE, layout=layout, want_g2=want_g2, **kw)  # (fetch: a NULL d_g2 writes nothing)
                host = GB.run_host(greg, batch, MG.GATE, layout=layout, want_g2=want_g2, **kw)
                assert (dev[2] is None) == (host[2] is None) == (not want_g2)
                GB.same(dev, exp, ("device", kw, layout, want_g2))
                GB.same(host, exp, ("host", kw, layout, want_g2))


# ---- 5: the pose records --------------------------------------------------------------------------------------------------------------
def test_pose_records_strides_and_statuses(pkg, greg):
    batch = GB.shared_batch(33)
    exp = GB.match_batch(batch, MG.GATE, knn=2)
    statuses = np.zeros(len(batch), np.int32); statuses[[1, 4]] = (SC_ENOHYP, SC_EINVAL)
    skipped = GB.match_batch(batch, MG.GATE, statuses=statuses, knn=2)
    assert skipped[3][4].tolist() == [0, 0] and exp[3][4, 0] > 0
    so, _ = batch.offsets()
    for dt in (None, GB.POSE64, GB.POSE80):
        rec = batch.poses(dt, statuses=statuses)  # without the flag the statuses are bytes like any other
        assert (48 if dt is None else dt.itemsize) in (48, 64, 80)
        GB.same(GB.run_device(pkg, greg, batch, MG.GATE, poses=rec, knn=2), exp, ("stride", rec.dtype.itemsize, "no flag"))
        if dt is None:
            continue
        got = GB.run_device(pkg, greg, batch, MG.GATE, poses=rec, flags=GB.STATUS, knn=2)
        GB.same(got, skipped, ("stride", dt.itemsize, "flag"))
        lo, hi = int(so[4]) * 2, int(so[5]) * 2
        assert (got[0][lo:hi] == GB.FILL_I).all() and (got[1][lo:hi] == np.float32(GB.FILL_F)).all() and (got[2][lo:hi] == np.float32(GB.FILL_F)).all()
        GB.same(GB.run_host(greg, batch, MG.GATE, poses=rec, flags=GB.STATUS, knn=2), skipped, ("host, stride", dt.itemsize, "flag"))
        # a skipped problem is not read: not its pose, not its descriptors
        rec2 = rec.copy(); rec2["Rt"][4] = np.nan
        bad = GB.with_scene(batch, 4, fsrc=np.full_like(batch.scenes[4].fsrc, np.nan))
        GB.same(GB.run_device(pkg, greg, bad, MG.GATE, poses=rec2, flags=GB.STATUS, knn=2), skipped, ("a skipped problem is not read", dt.itemsize))


# ---- 6: the chain and the features entry ------------------------------------------------------------------------------------------------
def _feature_batch():
    return GB.Batch([MG.Scene(s[0], s[1], s[2], s[3], np.zeros(12, np.float32)) for s in M.feature_scenes()])


def _features_outputs(nb, slots):
    import torch
    return dict(res=torch.zeros(nb * 80, dtype=torch.uint8, device="cuda"), corr=torch.full((slots, 2), GB.FILL_I, dtype=torch.int32, device="cuda"),
                d2=torch.full((slots,), GB.FILL_F, dtype=torch.float32, device="cuda"), count=torch.full((nb, 2), 9, dtype=torch.int32, device="cuda"),
                mask=torch.full((slots,), 7, dtype=torch.uint8, device="cuda"))


def test_the_chain_on_one_stream(pkg, greg):
    """register_batch_features_device, then match_guided_batch_device with d_pose = d_res (stride 80, the flag): no synchronisation
    in between; the second call equals the restatement fed the records read back afterwards"""
    import torch
    batch = _feature_batch()
    nb = len(batch)
    so, to = batch.offsets()
    slots = int(so[-1])
    mp, p = pkg.api.make_match_params(33, mutual=True), pkg.make_params(**M.KW)
    gate = 3 * M.KW["tau"]
    g = pkg.make_guide_params(gate, 0, GB.STATUS)
    d = GB.to_device(batch.packed())
    first, out = _features_outputs(nb, slots), GB.outputs(slots, nb)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    greg.set_stream(stream.cuda_stream)
    try:
        greg.register_batch_features_device(d[0].data_ptr(), d[1].data_ptr(), so, d[2].data_ptr(), d[3].data_ptr(), to, mp, p, first["res"].data_ptr(),
                                            first["corr"].data_ptr(), first["d2"].data_ptr(), first["count"].data_ptr(), first["mask"].data_ptr())
        greg.match_guided_batch_device(d[0].data_ptr(), d[1].data_ptr(), so, d[2].data_ptr(), d[3].data_ptr(), to, mp, g, first["res"].data_ptr(), 80,
                                       out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr())
        stream.synchronize()
    finally:
        greg.set_stream(None)
    rec = first["res"].cpu().numpy().view(GB.POSE80)
    got = GB.fetch(out, slots, nb)
    print("statuses", rec["status"].tolist(), "first n", first["count"].cpu().numpy()[:, 0].tolist(), "guided n", got[3][:, 0].tolist())
    assert len(batch.scenes[0].fsrc) == 2 and rec["status"][0] == SC_ENOHYP  # two keypoints: no hypothesis, hence skipped
    ok = np.flatnonzero(rec["status"] == SC_OK)
    assert len(ok) and (got[3][ok, 0] > 0).any()
    exp = GB.match_batch(batch, gate, statuses=rec["status"], poses=rec["Rt"], knn=1, mutual=True)
    GB.same(got, exp, "the chain")
    assert got[3][0].tolist() == [0, 0] and (got[3][rec["status"] != SC_OK] == 0).all()


@pytest.mark.parametrize("alias", [False, True])
def test_register_guided_batch_features_equals_the_composition(pkg, greg, alias):
    """the guided match, then register_batch on the gathered correspondences; once with d_pose aliasing d_res"""
    import torch
    batch = _feature_batch()
    nb = len(batch)
    so, to = batch.offsets()
    slots = int(so[-1])
    mp, p = pkg.api.make_match_params(33, mutual=True), pkg.make_params(**M.KW)
    gate = 3 * M.KW["tau"]
    g = pkg.make_guide_params(gate, 0, GB.STATUS)
    problems = [s.args()[:4] for s in batch.scenes]
    prior = greg.register_batch_features(problems, params=p, mutual=True)  # the poses the second pass is gated by
    rec = np.zeros(nb, GB.POSE80)
    for b, o in enumerate(prior):
        rec["Rt"][b] = np.concatenate([o["R"].ravel(), o["t"]]); rec["status"][b] = o["status"]
    assert SC_OK in rec["status"] and SC_ENOHYP in rec["status"]
    match = GB.run_device(pkg, greg, batch, gate, poses=rec, flags=GB.STATUS, knn=1, mutual=True)
    GB.same(match, GB.match_batch(batch, gate, statuses=rec["status"], poses=rec["Rt"], knn=1, mutual=True), "the match alone")
    d = GB.to_device(batch.packed())
    out, f = GB.outputs(slots, nb), _features_outputs(nb, slots)
    d_pose = f["res"] if alias else torch.zeros(nb * 80, dtype=torch.uint8, device="cuda")
    d_pose.copy_(torch.from_numpy(rec.view(np.uint8).reshape(-1)))
    torch.cuda.synchronize()
    greg.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        greg.register_guided_batch_features_device(d[0].data_ptr(), d[1].data_ptr(), so, d[2].data_ptr(), d[3].data_ptr(), to, mp, g, d_pose.data_ptr(),
                                                   80, p, f["res"].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                   out[3].data_ptr(), f["mask"].data_ptr())
        torch.cuda.synchronize()
    finally:
        greg.set_stream(None)
    got = GB.fetch(out, slots, nb)
    GB.same(got, match, ("the features entry's match", alias))
    res, mask = f["res"].cpu().numpy().view(GB.POSE80), f["mask"].cpu().numpy()
    big = [b for b in range(nb) if got[3][b, 0] >= 3]
    assert big and len(big) < nb
    gathered = [(batch.scenes[b].src_pts[got[0][int(so[b]): int(so[b]) + int(got[3][b, 0]), 0]],
                 batch.scenes[b].tgt_pts[got[0][int(so[b]): int(so[b]) + int(got[3][b, 0]), 1]]) for b in big]
    plain = greg.register_batch(gathered, params=p)
    for b, o in zip(big, plain):
        n = int(got[3][b, 0])
        print(b, "n", n, [int(res[f][b]) for f in FIELDS], "| register_batch", o["status"], o["stats"])
        assert [int(res[f][b]) for f in FIELDS] == [o["status"]] + [o["stats"][f] for f in FIELDS[1:]], b
        assert nan_equal_bits(res["Rt"][b], np.concatenate([o["R"].ravel(), o["t"]])), b
        assert np.array_equal(mask[int(so[b]): int(so[b]) + n], o["mask"]), b
    for b in set(range(nb)) - set(big):  # fewer than three matches (a skipped problem has none): SC_ENOHYP
        assert res["status"][b] == SC_ENOHYP and res["n"][b] == got[3][b, 0], b


# ---- 7: refusals reach the C entries ------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field(pkg):
    import torch
    batch = GB.Batch(GB.shared_batch(33).scenes[1:3])
    so, to = batch.offsets()
    slots = int(so[-1])
    G, Mp = pkg.make_guide_params, pkg.api.make_match_params
    r = pkg.Registrar(0)
    try:
        good = GB.run_device(pkg, r, batch, MG.GATE)
        d = GB.to_device(batch.packed() + (batch.poses(GB.POSE80).view(np.uint8).reshape(-1),))
        out, f = GB.outputs(slots, 2), _features_outputs(2, slots)
        torch.cuda.synchronize()

        def call(g=G(MG.GATE), stride=80, corr=out[0].data_ptr(), mp=Mp(33)):
            r.match_guided_batch_device(d[0].data_ptr(), d[1].data_ptr(), so, d[2].data_ptr(), d[3].data_ptr(), to, mp, g, d[4].data_ptr(), stride,
                                        corr, out[1].data_ptr(), None, out[3].data_ptr())

        def features(g, p):
            r.register_guided_batch_features_device(d[0].data_ptr(), d[1].data_ptr(), so, d[2].data_ptr(), d[3].data_ptr(), to, Mp(33), g,
                                                    d[4].data_ptr(), 80, p, f["res"].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), None,
                                                    out[3].data_ptr(), f["mask"].data_ptr())

        reserved = G(MG.GATE); reserved.reserved[1] = 1
        cases = [(lambda: call(stride=44), "pose_stride"), (lambda: call(stride=50), "pose_stride"),
                 (lambda: call(G(MG.GATE, 0, GB.STATUS), stride=48), "pose_stride"), (lambda: call(G(MG.GATE, 0, 2)), "flags"),
                 (lambda: call(G(MG.GATE, 0, 3)), "flags"), (lambda: call(G(0.0)), "gate"), (lambda: call(G(MG.GATE, 2)), "layout"),
                 (lambda: call(reserved), "reserved"), (lambda: call(corr=None), "d_corr"), (lambda: call(mp=Mp(33, knn=2, mutual=True)), "knn == 1"),
                 (lambda: features(G(MG.GATE, pkg.SC_SOA), pkg.make_params(**M.KW)), "layout"),
                 (lambda: features(G(MG.GATE), pkg.make_params(**M.KW, shard_world=2)), "shard_world")]
        for fn, word in cases:
            with pytest.raises(pkg.SacCotError) as e:
                fn()
            print(word, "|", e.value)
            assert e.value.status == SC_EINVAL and word in str(e.value), word
        S = pkg.synth
        _, c0 = S.make_config_scene("C0")
        ds, dt = torch.from_numpy(c0.src).cuda(), torch.from_numpy(c0.tgt).cuda()
        d_Rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_mask = torch.zeros(len(c0.src), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r.register_device_async(ds.data_ptr(), dt.data_ptr(), len(c0.src), pkg.make_params(**S.CONFIGS["C0"].params()), d_Rt.data_ptr(),
                                d_mask.data_ptr())
        with pytest.raises(pkg.SacCotError) as e:
            call()
        assert e.value.status == SC_EINVAL and "outstanding" in str(e.value)
        r.wait()
        torch.cuda.synchronize()
        # nothing was enqueued by a refused call: the outputs are as they were filled, and the context is as good as before
        assert (out[0].cpu().numpy() == GB.FILL_I).all() and (out[3].cpu().numpy() == 7).all()
        again = GB.run_device(pkg, r, batch, MG.GATE)
        for k in range(4):
            assert again[k].tobytes() == good[k].tobytes()
    finally:
        r.close()
