"""GPU: descriptor matching gated by several poses (include/saccot.h, sc_match_guided_poses / sc_match_guided_poses_device /
sc_register_guided_poses_features).

Every comparison is bit for bit against the numpy restatement (tests/match_guided_poses_ref.py): the correspondences, the bits of
the squared distances and of the smallest gate residuals, the labels, the count.  tests/test_match_guided_poses_abi.py checks, on the
CPU, that the restatement with one record is the single-pose one and that the shared scenes have what these tests use them for.
"""
import ctypes as C

import numpy as np
import pytest

import assign_ref as AR
import match_guided_poses_ref as MP
import match_guided_ref as MG
from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
MODES = MG.MODES
SHAPES = [(1, 1), (3, 5), (65, 63), (130, 129), (300, 333)]  # (130, 129): two row blocks x three column tiles, the last of each ragged
DIMS = [1, 33]
KS = [1, 2, 3, 64]
STATUS = 1  # SC_GUIDE_POSE_STATUS


@pytest.fixture(scope="module")
def greg(pkg):
    r = pkg.Registrar(0)
    yield r
    r.close()


def _same(got, exp, tag, label=True, g2=True):
    exp_c, exp_d, exp_g, exp_l = exp
    print(tag, "n", got["n"], "expected", len(exp_c))
    assert got["n"] == len(exp_c), tag
    assert np.array_equal(got["corr"], exp_c), tag
    assert got["d2"].view(np.uint32).tobytes() == exp_d.view(np.uint32).tobytes(), tag
    if g2:
        assert got["g2"].view(np.uint32).tobytes() == exp_g.view(np.uint32).tobytes(), tag
    if label:
        assert np.array_equal(got["label"], exp_l), tag


def _pts(sc, layout):
    return (sc.src_pts, sc.tgt_pts) if layout == 0 else (np.ascontiguousarray(sc.src_pts.T), np.ascontiguousarray(sc.tgt_pts.T))


def _host(r, sc, gate, pose=None, layout=0, flags=0, **kw):
    sp, tp = _pts(sc, layout)
    return r.match_guided_poses(sp, sc.fsrc, tp, sc.ftgt, sc.poses if pose is None else pose, gate=gate, layout=layout, flags=flags, **kw)


def _device(pkg, r, sc, gate, pose=None, flags=0, want_g2=True, want_label=True, layout=0, pose_by_copy=False, **kw):
    """sc_match_guided_poses_device on the current torch stream -> dict(n, flag, corr, d2, g2 or None, label or None), cut at the count"""
    import torch
    dev = torch.device("cuda:0")
    ns, nt = sc.fsrc.shape[0], sc.ftgt.shape[0]
    m, g = pkg.api.make_match_params(sc.fsrc.shape[1], **kw), pkg.make_guide_params(gate, layout, flags)
    cap = ns * m.knn
    sp, tp = _pts(sc, layout)
    d = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev) for x in (sp, sc.fsrc, tp, sc.ftgt)]
    rec, stride = pkg.Registrar._pose_records(sc.poses if pose is None else pose)
    rec_host = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).pin_memory()
    d_pose = torch.zeros(rec_host.numel(), dtype=torch.uint8, device=dev) if pose_by_copy else rec_host.to(dev)
    d_corr = torch.full((cap, 2), -1, dtype=torch.int32, device=dev); d_d2 = torch.zeros(cap, dtype=torch.float32, device=dev)
    d_g2 = torch.full((cap,), -1.0, dtype=torch.float32, device=dev); d_lab = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    d_cnt = torch.full((2,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        if pose_by_copy:  # the records arrive by a copy enqueued on the same stream immediately before the call: no synchronisation
            d_pose.copy_(rec_host, non_blocking=True)
        r.match_guided_poses_device(d[0].data_ptr(), d[1].data_ptr(), ns, d[2].data_ptr(), d[3].data_ptr(), nt, m, g, d_pose.data_ptr(),
                                    stride, len(rec), d_corr.data_ptr(), d_d2.data_ptr(), d_g2.data_ptr() if want_g2 else None,
                                    d_lab.data_ptr() if want_label else None, d_cnt.data_ptr())
        torch.cuda.synchronize()
    finally:
        r.set_stream(None)
    n, flag = d_cnt.cpu().tolist()
    if not want_g2:
        assert (d_g2.cpu().numpy() == -1.0).all()
    if not want_label:
        assert (d_lab.cpu().numpy() == -7).all()
    assert (d_corr.cpu().numpy()[n:] == -1).all() and (d_lab.cpu().numpy()[n:] == -7).all()  # nothing is written behind the count
    assert rec_host.numpy().tobytes() == (d_pose.cpu().numpy().tobytes())  # the records are read, never written
    return dict(n=n, flag=flag, corr=d_corr.cpu().numpy()[:n], d2=d_d2.cpu().numpy()[:n], g2=d_g2.cpu().numpy()[:n] if want_g2 else None,
                label=d_lab.cpu().numpy()[:n] if want_label else None)


def _raw(pkg, r, sc, gate, pose, stride, n_poses, flags=0, **kw):
    """the host entry itself -> (status, n, the message): what the wrapper turns into an exception"""
    L = pkg.load_library()
    f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    ns, nt = sc.fsrc.shape[0], sc.ftgt.shape[0]
    m, g = pkg.api.make_match_params(sc.fsrc.shape[1], **kw), pkg.make_guide_params(gate, 0, flags)
    corr = np.zeros((ns * m.knn, 2), np.int32); d2 = np.zeros(ns * m.knn, np.float32); n = C.c_uint32(7)
    keep = [np.ascontiguousarray(x, np.float32) for x in (sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt)]
    pose = None if pose is None else np.ascontiguousarray(pose)
    rc = L.sc_match_guided_poses(r._h, f32(keep[0]), f32(keep[1]), ns, f32(keep[2]), f32(keep[3]), nt, C.byref(m), C.byref(g),
                                 None if pose is None else pose.ctypes.data_as(C.c_void_p), stride, n_poses,
                                 corr.ctypes.data_as(C.POINTER(C.c_int32)), f32(d2), None, None, C.byref(n))
    return rc, n.value, L.sc_last_error(r._h).decode()


# ---- 1: shapes x descriptor lengths x numbers of records x modes -------------------------------------------------
@pytest.mark.parametrize("ns,nt", SHAPES)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("K", KS)
def test_poses_match_equals_the_restatement(pkg, greg, ns, nt, D, K):
    sc = MP.shared_scene(ns, nt, D, K)
    prob = MP.Problem(*sc.args(), MP.GATE)
    for kw in MODES:
        _same(_host(greg, sc, MP.GATE, **kw), prob.match(**kw), (ns, nt, D, K, kw))
    if ns >= 130 and K <= 3:  # the gate bites, and more than one record labels
        lab = prob.match(knn=1)[3]
        assert not prob.adm.all() and prob.adm.any() and (K == 1 or len(np.unique(lab)) == K)
    # the device form, d_g2 and d_label given or NULL independently
    exp = prob.match(knn=4)
    for want_g2, want_label in ((True, True), (True, False), (False, True), (False, False)):
        got = _device(pkg, greg, sc, MP.GATE, want_g2=want_g2, want_label=want_label, knn=4)
        assert got["flag"] == 0
        _same(got, exp, ("device", ns, nt, D, K, want_g2, want_label), label=want_label, g2=want_g2)
    none = _device(pkg, greg, sc, MG.GATE_NOTHING, knn=2)
    assert (none["n"], none["flag"]) == (0, 0)  # nothing admissible is no error


# ---- 2: one record is sc_match_guided_device ---------------------------------------------------------------------
def _single_device(pkg, r, sc, gate, Rt, **kw):
    import torch
    dev = torch.device("cuda:0")
    ns, nt = sc.fsrc.shape[0], sc.ftgt.shape[0]
    m, g = pkg.api.make_match_params(sc.fsrc.shape[1], **kw), pkg.make_guide_params(gate)
    cap = ns * m.knn
    d = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev) for x in (sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, Rt)]
    d_corr = torch.full((cap, 2), -1, dtype=torch.int32, device=dev); d_d2 = torch.zeros(cap, dtype=torch.float32, device=dev)
    d_g2 = torch.zeros(cap, dtype=torch.float32, device=dev); d_cnt = torch.full((2,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        r.match_guided_device(d[0].data_ptr(), d[1].data_ptr(), ns, d[2].data_ptr(), d[3].data_ptr(), nt, m, g, d[4].data_ptr(),
                              d_corr.data_ptr(), d_d2.data_ptr(), d_g2.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
    finally:
        r.set_stream(None)
    n, flag = d_cnt.cpu().tolist()
    return dict(n=n, flag=flag, corr=d_corr.cpu().numpy()[:n], d2=d_d2.cpu().numpy()[:n], g2=d_g2.cpu().numpy()[:n])


@pytest.mark.parametrize("ns,nt,D", [(130, 129, 33), (300, 333, 33), (65, 63, 1)])
def test_one_record_equals_the_single_pose_entry(pkg, greg, ns, nt, D):
    sc = MP.shared_scene(ns, nt, D, 3)
    for k in (0, 2):
        one = sc.with_poses(sc.poses[k])
        for kw in MODES:
            got = _device(pkg, greg, one, MP.GATE, **kw)
            exp = _single_device(pkg, greg, sc, MP.GATE, sc.poses[k], **kw)
            assert (got["n"], got["flag"]) == (exp["n"], exp["flag"]) and (ns < 130 or got["n"] > 0), (k, kw)
            for f in ("corr", "d2", "g2"):
                assert got[f].tobytes() == exp[f].tobytes(), (k, kw, f)
            assert not got["label"].any(), (k, kw)
    # ... a non-finite pose included: the flag and n = 0
    bad = sc.poses[0].copy(); bad[7] = np.nan
    got, exp = _device(pkg, greg, sc.with_poses(bad), MP.GATE), _single_device(pkg, greg, sc, MP.GATE, bad)
    assert (got["n"], got["flag"]) == (exp["n"], exp["flag"]) == (0, 1)


# ---- 3: the order of the records ---------------------------------------------------------------------------------
def test_permuted_records_permute_the_labels_and_nothing_else(pkg, greg):
    sc = MP.shared_scene(300, 333, 33, 3)
    perm = np.array([2, 0, 1])  # the new list's record k is the old record perm[k]
    inv = np.argsort(perm)
    for kw in MODES:
        a, b = _host(greg, sc, MP.GATE, **kw), _host(greg, sc, MP.GATE, pose=sc.poses[perm], **kw)
        assert a["n"] == b["n"] > 0 and len(np.unique(a["label"])) == 3, kw
        for f in ("corr", "d2", "g2"):
            assert a[f].tobytes() == b[f].tobytes(), (kw, f)
        assert np.array_equal(b["label"], inv[a["label"]]), kw


def test_identical_records_never_yield_the_higher_index(pkg, greg):
    sc = MP.tie_scene(300, 333, 33)
    prob = MP.Problem(*sc.args(), MP.GATE)
    for kw in MODES:
        got = _host(greg, sc, MP.GATE, **kw)
        _same(got, prob.match(**kw), ("tie", kw))
        assert (got["label"] != 1).all() and (got["label"] == 0).any() and (got["label"] == 2).any(), kw
    dev = _device(pkg, greg, sc, MP.GATE, knn=4)
    _same(dev, prob.match(knn=4), "tie, the device form")


# ---- 4: SC_GUIDE_POSE_STATUS -------------------------------------------------------------------------------------
def test_records_with_a_status(pkg, greg):
    sc = MP.shared_scene(130, 129, 33, 3)
    prob = MP.Problem(*sc.args(), MP.GATE)
    ident = AR.rt_of(np.eye(3), np.zeros(3))
    nan_rt = np.full(12, np.nan, np.float32)
    shifted = np.array([0, 2, 3])  # with a skipped record at index 1, the old record k is the new record shifted[k]
    modes = [dict(knn=1), dict(knn=4), dict(knn=1, mutual=True), dict(knn=1, ratio=0.8)]
    for what, skipped in (("identity", ident), ("NaN", nan_rt)):
        four = np.stack([sc.poses[0], skipped, sc.poses[1], sc.poses[2]])
        rec = MP.records(four, status=[SC_OK, SC_ENOHYP, SC_OK, SC_OK])
        assert rec.dtype.itemsize == 80
        for kw in modes:
            c, d, g, lab = prob.match(**kw)
            exp = (c, d, g, shifted[lab].astype(np.int32))
            _same(_host(greg, sc, MP.GATE, pose=rec, flags=STATUS, **kw), exp, ("skipped", what, "host", kw))
            dev = _device(pkg, greg, sc, MP.GATE, pose=rec, flags=STATUS, **kw)
            assert dev["flag"] == 0
            _same(dev, exp, ("skipped", what, "device", kw))
    # all statuses SC_OK with the flag: the plain result
    _same(_host(greg, sc, MP.GATE, pose=MP.records(sc.poses), flags=STATUS, knn=2), prob.match(knn=2), "every record used")
    # the same NaN record without the flag is read: count[1] = 1 and n = 0 (stride 80, the status ignored)
    dev = _device(pkg, greg, sc, MP.GATE, pose=rec, flags=0)
    assert (dev["n"], dev["flag"]) == (0, 1)
    rc, n, text = _raw(pkg, greg, sc, MP.GATE, rec, 80, 4)
    assert rc == SC_EINVAL and n == 0 and "non-finite" in text and "pose" in text
    # a NaN in a USED record with the flag raises it as well
    used_bad = MP.records(np.stack([sc.poses[0], nan_rt]), status=[SC_OK, SC_OK])
    dev = _device(pkg, greg, sc, MP.GATE, pose=used_bad, flags=STATUS)
    assert (dev["n"], dev["flag"]) == (0, 1)
    # every record skipped: n = 0, no flag
    none = MP.records(four, status=[SC_ENOHYP, SC_EINVAL, 7, -100])
    for kw in modes:
        dev = _device(pkg, greg, sc, MP.GATE, pose=none, flags=STATUS, **kw)
        assert (dev["n"], dev["flag"]) == (0, 0), kw
    assert _host(greg, sc, MP.GATE, pose=none, flags=STATUS)["n"] == 0
    # ... but a non-finite descriptor is still reported
    bad = MP.Scene(sc.src_pts, sc.fsrc.copy(), sc.tgt_pts, sc.ftgt, sc.poses)
    bad.fsrc[129, 32] = np.inf
    dev = _device(pkg, greg, bad, MP.GATE, pose=none, flags=STATUS)
    assert (dev["n"], dev["flag"]) == (0, 1)


# ---- 5: skipped tiles and the flag -------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cluster", "two_tiles"])
def test_skipped_tiles_and_the_non_finite_flag(pkg, greg, which):
    sc = MP.cluster_scene() if which == "cluster" else MP.two_tiles_scene()
    prob = MP.Problem(*sc.args(), MP.GATE)
    modes = [dict(knn=4), dict(knn=1, mutual=True)] if which == "two_tiles" else MODES
    for kw in modes:
        _same(_host(greg, sc, MP.GATE, **kw), prob.match(**kw), (which, kw))
    dropped = 128 if which == "cluster" else 2 * 64 + 3  # a target column in a tile that every record drops
    assert not prob.adm[:, (dropped // 64) * 64:(dropped // 64 + 1) * 64].any()
    for arr, pos, val in (("ftgt", (dropped, sc.ftgt.shape[1] - 1), np.nan), ("ftgt", (dropped, 0), -np.inf), ("tgt_pts", (dropped, 1), np.inf)):
        bad = MP.Scene(sc.src_pts.copy(), sc.fsrc.copy(), sc.tgt_pts.copy(), sc.ftgt.copy(), sc.poses)
        getattr(bad, arr)[pos] = val
        for kw in (dict(knn=1), dict(knn=1, mutual=True)):
            dev = _device(pkg, greg, bad, MP.GATE, **kw)
            assert (dev["n"], dev["flag"]) == (0, 1), (arr, pos, val, kw)
        rc, n, text = _raw(pkg, greg, bad, MP.GATE, sc.poses, 48, 3)
        assert rc == SC_EINVAL and n == 0 and "non-finite" in text, (arr, pos, val)
    # a non-finite value inside a skipped record raises nothing: the result is that of the used records
    poses = sc.poses.copy(); poses[1, 4] = np.nan
    rec = MP.records(poses, status=[SC_OK, SC_ENOHYP, SC_OK])
    used = MP.Problem(*sc.args(), MP.GATE, used=[True, False, True])
    for kw in modes[:2]:
        dev = _device(pkg, greg, sc, MP.GATE, pose=rec, flags=STATUS, **kw)
        assert dev["flag"] == 0 and dev["n"] > 0
        _same(dev, used.match(**kw), (which, "a skipped record with a NaN", kw))


# ---- 6: the boundary of the gate ---------------------------------------------------------------------------------
def test_the_boundary_of_the_gate(pkg, greg):
    half = np.float32(0.5)
    below = np.nextafter(half, np.float32(0))
    poses = np.stack([MP.shift([0, 80.0, 0]), MP.shift([0, 0, 0])])  # the smallest residual is the second record's
    sc = MP.Scene(np.zeros((1, 3), np.float32), np.zeros((1, 1), np.float32), np.array([[half, 0, 0], [below, 0, 0]], np.float32),
                  np.array([[0.0], [1.0]], np.float32), poses)
    prob = MP.Problem(*sc.args(), 0.5)
    assert prob.g2[0, 0] == np.float32(0.25) == MG.gate2_of(0.5) and prob.g2[0, 1] < np.float32(0.25)
    assert prob.adm.tolist() == [[False, True]] and prob.label.tolist() == [[1, 1]]
    for kw in MODES:
        got = _host(greg, sc, 0.5, **kw)
        _same(got, prob.match(**kw), ("g2 == gate2 is not admissible", kw))
        # (the nearer descriptor sits at the inadmissible target: the blind match would be (0, 0))
        assert got["corr"].tolist() == [[0, 1]] and got["label"].tolist() == [1] and got["g2"][0] < np.float32(0.25), kw
    # finite records whose residuals are NaN or inf admit nothing and raise no flag; beside an ordinary record they change nothing
    big = MP.shared_scene(130, 129, 33, 2)
    hostile = big.with_poses(np.stack([AR.hostile(), AR.hostile()]))
    for gate in (MP.GATE, MG.GATE_ALL, 3e38):
        dev = _device(pkg, greg, hostile, gate, knn=4)
        assert (dev["n"], dev["flag"]) == (0, 0), gate
    mixed = big.with_poses(np.stack([AR.hostile(), big.poses[1]]))
    exp = MP.Problem(*mixed.args(), MP.GATE).match(knn=4)
    assert len(exp[0]) and (exp[3] == 1).all()
    _same(_host(greg, mixed, MP.GATE, knn=4), exp, "a hostile record beside an ordinary one")


# ---- 7: forms and contexts agree ---------------------------------------------------------------------------------
def test_forms_and_contexts_agree(pkg, greg):
    sc = MP.shared_scene(300, 333, 33, 3)
    for kw in (dict(knn=1), dict(knn=4), dict(knn=1, mutual=True), dict(knn=1, ratio=0.8), dict(knn=1, mutual=True, ratio=0.9)):
        host = _host(greg, sc, MP.GATE, **kw)
        _same(host, MP.match(*sc.args(), MP.GATE, **kw), ("host form", kw))
        again = _host(greg, sc, MP.GATE, **kw)
        soa = _host(greg, sc, MP.GATE, layout=pkg.SC_SOA, **kw)
        fresh = pkg.Registrar(0)
        try:
            other = _host(fresh, sc, MP.GATE, **kw)
            by_copy = _device(pkg, fresh, sc, MP.GATE, pose_by_copy=True, **kw)
            soa_dev = _device(pkg, fresh, sc, MP.GATE, layout=pkg.SC_SOA, pose=MP.records(sc.poses), **kw)  # (stride 80, no flag)
        finally:
            fresh.close()
        assert (by_copy["n"], by_copy["flag"]) == (soa_dev["n"], soa_dev["flag"]) == (host["n"], 0), kw
        for x in (again, soa, other, by_copy, soa_dev):
            for f in ("corr", "d2", "g2", "label"):
                assert x[f].tobytes() == host[f].tobytes(), (kw, f)


# ---- 8: descriptors and K poses in, (R, t), correspondences, labels and mask out ---------------------------------
def _flat(res):
    return np.concatenate([res["R"].ravel(), res["t"]])


def test_register_guided_poses_features_equals_the_composition(pkg):
    S = pkg.synth
    cfg = S.CONFIGS["C0"]
    sc = S.make_feature_scene(cfg, 300, 32, 1.0)
    kw = cfg.params()
    p = pkg.make_params(**kw)
    gate = 3 * cfg.tau
    truth = AR.rt_of(sc.R_gt, sc.t_gt)
    near = AR.perturbed(truth, 2, 17, angle=0.05, shift=cfg.tau / 2)  # two priors a few degrees off the true pose, in different directions
    rng = np.random.default_rng(5)
    poses = np.stack([near[0], AR.rt_of(*MG.random_pose(rng)), near[1]])
    scene = MP.Scene(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, poses)
    prob = MP.Problem(*scene.args(), gate)
    r, r2 = pkg.Registrar(0), pkg.Registrar(0)
    try:
        for mode in (dict(), dict(mutual=True), dict(ratio=0.9)):
            exp = prob.match(knn=1, **mode)
            got = r.register_guided_poses_features(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, poses, gate=gate, params=p, **mode)
            _same(got, exp, ("register_guided_poses_features", mode))
            match = _device(pkg, r2, scene, gate, **mode)
            assert match["corr"].tobytes() == got["corr"].tobytes() and match["label"].tobytes() == got["label"].tobytes()
            src = np.ascontiguousarray(sc.src_pts[match["corr"][:, 0]]); tgt = np.ascontiguousarray(sc.tgt_pts[match["corr"][:, 1]])
            plain = r2.register(src, tgt, params=p)
            per = np.bincount(got["label"], minlength=3)
            print(mode, "n", got["n"], "per record", per.tolist(), "status", got["status"], "winner", got["stats"]["best_count"])
            assert got["n"] >= 3 and per[0] >= 3 and per[2] >= 3
            assert plain["status"] == got["status"] == SC_OK and np.array_equal(plain["mask"], got["mask"]), mode
            assert nan_equal_bits(_flat(plain), _flat(got)), mode
            for k in ("n", "edges", "tri_total", "tri_kept", "tri_scored", "best_rank", "best_count"):
                assert plain["stats"][k] == got["stats"][k], (mode, k)
            # the call leaves that frame: the records are refitted on their own entries, by the labels as they came back
            pol, masks = r.polish_poses(poses, sel=got["label"], sel_mode=pkg.SC_POLISH_POSES_SEL_LABEL, max_iter=4)
            pol2, masks2 = r2.polish_poses(poses, sel=match["label"], sel_mode=pkg.SC_POLISH_POSES_SEL_LABEL, max_iter=4)
            assert pol.tobytes() == pol2.tobytes() and np.array_equal(masks, masks2), mode
            for k in range(3):
                if per[k] >= 3:
                    assert pol["status"][k] == SC_OK, (mode, k)
                assert not masks[k][got["label"] != k].any(), (mode, k)  # a record's mask stays inside its label
            info = r.pose_info_frame(pol, sel=got["label"], sel_mode=pkg.SC_POSE_INFO_SEL_LABEL, flags=pkg.SC_POSE_INFO_STATUS)
            assert len(info) == 3
        # SoA keypoints give the same answer
        soa = r.register_guided_poses_features(np.ascontiguousarray(sc.src_pts.T), sc.fsrc, np.ascontiguousarray(sc.tgt_pts.T), sc.ftgt, poses,
                                               gate=gate, ratio=0.9, layout=pkg.SC_SOA, **kw)
        assert soa["corr"].tobytes() == got["corr"].tobytes() and soa["label"].tobytes() == got["label"].tobytes()
        assert np.array_equal(soa["mask"], got["mask"]) and nan_equal_bits(_flat(soa), _flat(got))
        # fewer than three matches: SC_ENOHYP, R = I, the matches still returned; no frame is left
        two = r.register_guided_poses_features(sc.src_pts[:2], sc.fsrc[:2], sc.tgt_pts, sc.ftgt, poses, gate=gate, params=p)
        exp = MP.match(sc.src_pts[:2], sc.fsrc[:2], sc.tgt_pts, sc.ftgt, poses, gate)
        assert two["status"] == SC_ENOHYP and two["n"] == len(exp[0]) < 3 and np.array_equal(two["corr"], exp[0])
        assert np.array_equal(two["label"], exp[3])
        assert np.array_equal(two["R"], np.eye(3, dtype=np.float32)) and not two["t"].any()
        with pytest.raises(pkg.SacCotError) as e:
            r.peel()
        assert e.value.status == SC_EINVAL
    finally:
        r.close(); r2.close()


# ---- 9: refusals reach the C entries -----------------------------------------------------------------------------
def test_refusals_name_the_field(pkg):
    import torch
    sc = MP.shared_scene(65, 63, 33, 3)
    G, M = pkg.make_guide_params, pkg.api.make_match_params
    r = pkg.Registrar(0)
    try:
        good = _host(r, sc, MP.GATE)
        rec = MP.records(sc.poses)
        for stride, n_poses, flags, word in ((48, 0, 0, "n_poses"), (48, 65, 0, "n_poses"), (80, 65, STATUS, "n_poses"), (44, 3, 0, "pose_stride"),
                                             (46, 3, 0, "pose_stride"), (50, 3, 0, "pose_stride"), (48, 3, STATUS, "pose_stride"),
                                             (80, 3, 2, "flags"), (80, 3, 3, "flags")):
            rc, n, text = _raw(pkg, r, sc, MP.GATE, rec, stride, n_poses, flags)
            assert rc == SC_EINVAL and n == 0 and word in text and "sc_match_guided_poses" in text, (stride, n_poses, flags, text)
        rc, n, text = _raw(pkg, r, sc, MP.GATE, None, 48, 3)
        assert rc == SC_EINVAL and "pose is NULL" in text
        # everything sc_match_guided refuses
        wrong_size = G(0.1); wrong_size.size = 28
        reserved = G(0.1); reserved.reserved[2] = 1
        for g, word in ((G(0.0), "gate"), (G(float("nan")), "gate"), (G(float("inf")), "gate"), (G(0.1, 2), "layout"), (wrong_size, "size"),
                        (reserved, "reserved")):
            with pytest.raises(pkg.SacCotError) as e:
                r.match_guided_poses(*sc.args(), gparams=g)
            assert e.value.status == SC_EINVAL and word in str(e.value) and "sc_match_guided_poses" in str(e.value), word
        with pytest.raises(pkg.SacCotError) as e:  # every rule of sc_match_params
            r.match_guided_poses(*sc.args(), gate=0.1, mparams=M(33, knn=2, mutual=True))
        assert e.value.status == SC_EINVAL and "knn == 1" in str(e.value)
        with pytest.raises(pkg.SacCotError) as e:  # the features entry: one layout
            r.register_guided_poses_features(np.ascontiguousarray(sc.src_pts.T), sc.fsrc, np.ascontiguousarray(sc.tgt_pts.T), sc.ftgt, sc.poses,
                                             gparams=G(0.1, pkg.SC_SOA), params=pkg.make_params())
        assert e.value.status == SC_EINVAL and "layout" in str(e.value)
        # the device entry: a NULL d_pose, a NULL d_corr, then a call outstanding on the context
        dev = torch.device("cuda:0")
        d = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev) for x in sc.args()]
        d_corr = torch.zeros((65, 2), dtype=torch.int32, device=dev); d_d2 = torch.zeros(65, dtype=torch.float32, device=dev)
        d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def call(pose_ptr, corr_ptr, g=G(0.1), n_poses=3):
            r.match_guided_poses_device(d[0].data_ptr(), d[1].data_ptr(), 65, d[2].data_ptr(), d[3].data_ptr(), 63, M(33), g, pose_ptr, 48,
                                        n_poses, corr_ptr, d_d2.data_ptr(), None, None, d_cnt.data_ptr())

        for args, word in (((None, d_corr.data_ptr()), "d_pose"), ((d[4].data_ptr(), None), "d_corr"),
                           ((d[4].data_ptr(), d_corr.data_ptr(), G(0.1, 7)), "layout"), ((d[4].data_ptr(), d_corr.data_ptr(), G(0.1), 65), "n_poses")):
            with pytest.raises(pkg.SacCotError) as e:
                call(*args)
            assert e.value.status == SC_EINVAL and word in str(e.value), word
        # sc_match_guided_device still refuses SC_GUIDE_POSE_STATUS
        with pytest.raises(pkg.SacCotError) as e:
            r.match_guided_device(d[0].data_ptr(), d[1].data_ptr(), 65, d[2].data_ptr(), d[3].data_ptr(), 63, M(33), G(0.1, 0, STATUS),
                                  d[4].data_ptr(), d_corr.data_ptr(), d_d2.data_ptr(), None, d_cnt.data_ptr())
        assert e.value.status == SC_EINVAL and "flags" in str(e.value)
        S = pkg.synth
        _, c0 = S.make_config_scene("C0")
        ds, dt = torch.from_numpy(c0.src).to(dev), torch.from_numpy(c0.tgt).to(dev)
        d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(len(c0.src), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        r.register_device_async(ds.data_ptr(), dt.data_ptr(), len(c0.src), pkg.make_params(**S.CONFIGS["C0"].params()), d_Rt.data_ptr(),
                                d_mask.data_ptr())
        with pytest.raises(pkg.SacCotError) as e:
            call(d[4].data_ptr(), d_corr.data_ptr())
        assert e.value.status == SC_EINVAL and "outstanding" in str(e.value)
        r.wait()
        # nothing was enqueued by a refused call, and the context is as good as before
        again = _host(r, sc, MP.GATE)
        for f in ("corr", "d2", "g2", "label"):
            assert again[f].tobytes() == good[f].tobytes()
    finally:
        r.close()
