"""GPU: descriptor matching gated by a pose prior (include/saccot.h, sc_match_guided / sc_match_guided_device /
sc_register_guided_features).

Every comparison is bit for bit against the numpy restatement (tests/match_guided_ref.py): the correspondences, the bits of the
squared distances and of the gate residuals, the count.  tests/test_match_guided_abi.py checks, on the CPU, that the restatement with
an open gate is match_ref and that the shared scene has rows with no, one and several admissible candidates.
"""
import ctypes as C

import numpy as np
import pytest

import assign_ref as AR
import match_guided_ref as MG
from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
MODES = MG.MODES
SHAPES = [(1, 1), (3, 5), (65, 63), (130, 129), (300, 333)]  # (130, 129): two row blocks x three column tiles, the last of each ragged
DIMS = [1, 33, 352]                                          # 33: 16 + 16 + 1 components


@pytest.fixture(scope="module")
def greg(pkg):
    r = pkg.Registrar(0)
    yield r
    r.close()


def _same(got, exp, tag):
    exp_c, exp_d, exp_g = exp
    print(tag, "n", got["n"], "expected", len(exp_c))
    assert got["n"] == len(exp_c), tag
    assert np.array_equal(got["corr"], exp_c), tag
    assert got["d2"].view(np.uint32).tobytes() == exp_d.view(np.uint32).tobytes(), tag
    assert got["g2"].view(np.uint32).tobytes() == exp_g.view(np.uint32).tobytes(), tag


def _check(pkg, r, sc, gate, modes=MODES, layout=0, what=""):
    prob = MG.Problem(*sc.args(), gate)
    sp, tp = (sc.src_pts, sc.tgt_pts) if layout == 0 else (np.ascontiguousarray(sc.src_pts.T), np.ascontiguousarray(sc.tgt_pts.T))
    out = {}
    for kw in modes:
        got = r.match_guided(sp, sc.fsrc, tp, sc.ftgt, sc.Rt, gate=gate, layout=layout, **kw)
        _same(got, prob.match(**kw), (what, sc.fsrc.shape, sc.ftgt.shape, gate, layout, kw))
        out[tuple(sorted(kw.items()))] = got
    return prob, out


def _raw(pkg, r, sc, gate, Rt=None, **kw):
    """the host entry itself -> (status, n, the message): what the wrapper turns into an exception"""
    L = pkg.load_library()
    f32 = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    ns, nt = sc.fsrc.shape[0], sc.ftgt.shape[0]
    m, g = pkg.api.make_match_params(sc.fsrc.shape[1], **kw), pkg.make_guide_params(gate)
    corr = np.zeros((ns * m.knn, 2), np.int32); d2 = np.zeros(ns * m.knn, np.float32); n = C.c_uint32(7)
    keep = [np.ascontiguousarray(x, np.float32) for x in (sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, sc.Rt if Rt is None else Rt)]
    rc = L.sc_match_guided(r._h, f32(keep[0]), f32(keep[1]), ns, f32(keep[2]), f32(keep[3]), nt, C.byref(m), C.byref(g), f32(keep[4]),
                           corr.ctypes.data_as(C.POINTER(C.c_int32)), f32(d2), None, C.byref(n))
    return rc, n.value, L.sc_last_error(r._h).decode()


def _device(pkg, r, sc, gate, Rt=None, want_g2=True, layout=0, pose_by_copy=False, **kw):
    """sc_match_guided_device on the current torch stream -> (count pair, corr, d2, g2 or None), cut at the count"""
    import torch
    dev = torch.device("cuda:0")
    ns, nt = sc.fsrc.shape[0], sc.ftgt.shape[0]
    m, g = pkg.api.make_match_params(sc.fsrc.shape[1], **kw), pkg.make_guide_params(gate, layout)
    cap = ns * m.knn
    sp, tp = (sc.src_pts, sc.tgt_pts) if layout == 0 else (np.ascontiguousarray(sc.src_pts.T), np.ascontiguousarray(sc.tgt_pts.T))
    d = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev) for x in (sp, sc.fsrc, tp, sc.ftgt)]
    rt_host = torch.from_numpy(np.ascontiguousarray(sc.Rt if Rt is None else Rt, np.float32)).pin_memory()
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev) if pose_by_copy else rt_host.to(dev)
    d_corr = torch.full((cap, 2), -1, dtype=torch.int32, device=dev); d_d2 = torch.zeros(cap, dtype=torch.float32, device=dev)
    d_g2 = torch.full((cap,), -1.0, dtype=torch.float32, device=dev)
    d_cnt = torch.full((2,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        if pose_by_copy:  # the pose arrives by a copy enqueued on the same stream immediately before the call: no synchronisation
            d_Rt.copy_(rt_host, non_blocking=True)
        r.match_guided_device(d[0].data_ptr(), d[1].data_ptr(), ns, d[2].data_ptr(), d[3].data_ptr(), nt, m, g, d_Rt.data_ptr(),
                              d_corr.data_ptr(), d_d2.data_ptr(), d_g2.data_ptr() if want_g2 else None, d_cnt.data_ptr())
        torch.cuda.synchronize()
    finally:
        r.set_stream(None)
    n, flag = d_cnt.cpu().tolist()
    if not want_g2:
        assert (d_g2.cpu().numpy() == -1.0).all()
    assert (d_corr.cpu().numpy()[n:] == -1).all()  # nothing is written behind the count
    return (n, flag), d_corr.cpu().numpy()[:n], d_d2.cpu().numpy()[:n], (d_g2.cpu().numpy()[:n] if want_g2 else None)


# ---- 1: shapes x descriptor lengths x modes x gates --------------------------------------------------------------
@pytest.mark.parametrize("ns,nt", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_guided_match_equals_the_restatement(pkg, greg, ns, nt, D):
    sc = MG.shared_scene(ns, nt, D)
    prob, got = _check(pkg, greg, sc, MG.GATE)
    if ns >= 130:  # the gate bites: some rows have nothing, something is kept
        assert 0 < got[(("knn", 1),)]["n"] < ns and not prob.adm.all() and prob.adm.any()
    _, none = _check(pkg, greg, sc, MG.GATE_NOTHING, what="nothing admissible")
    assert all(g["n"] == 0 for g in none.values())
    flag = _device(pkg, greg, sc, MG.GATE_NOTHING)[0]
    assert flag == (0, 0)  # ... and that is no error
    if (ns, nt) == (130, 129):
        _check(pkg, greg, sc, MG.GATE, layout=pkg.SC_SOA, what="SoA points")
        cnt, corr, d2, g2 = _device(pkg, greg, sc, MG.GATE, layout=pkg.SC_SOA, knn=4)
        _same(dict(n=cnt[0], corr=corr, d2=d2, g2=g2), prob.match(knn=4), "SoA points, the device form")


# ---- 2: more than one tile per slice -----------------------------------------------------------------------------
def test_two_tiles_per_slice_one_skipped(pkg, greg):
    """(5, 70 000): 1094 column tiles in 547 slices of two.  The target tiles alternate between the sources' cluster and one far
    away in a period of three, so slices hold (far, near), (far, far), (near, far), ... : a skipped tile before and after a computed one"""
    ns, nt, D = 5, 70000, 2
    near, far = np.zeros(3), np.array([40.0, -30.0, 20.0])
    tile = np.arange(nt) // 64
    ct = np.where((tile % 3 == 1)[:, None], near[None, :], far[None, :])
    sc = MG.clusters(301, np.tile(near, (ns, 1)), ct, D)
    prob, got = _check(pkg, greg, sc, MG.GATE, modes=[dict(knn=4), dict(knn=1, mutual=True)], what="two tiles per slice")
    col_tiles = np.unique(np.flatnonzero(prob.adm.any(axis=0)) // 64)
    assert len(col_tiles) > 300 and (col_tiles % 3 == 1).all()  # whole tiles are admissible or not
    assert got[(("knn", 4),)]["n"] == 4 * ns


# ---- 3: the skip path and the flag -------------------------------------------------------------------------------
def _skip_scene(D=33):
    """source rows 0..127 in cluster A, 128..255 in B, 256..383 in C (no target near: every tile of that row block is skipped);
    target columns 0..63 near B, 64..127 near A, 128..191 in a cluster of their own (skipped by every row block)"""
    A, B, Cc, Dd = np.array([0.0, 0, 0]), np.array([50.0, 0, 0]), np.array([0, 80.0, 0]), np.array([0, 0, -90.0])
    cs = np.concatenate([np.tile(A, (128, 1)), np.tile(B, (128, 1)), np.tile(Cc, (128, 1))])
    ct = np.concatenate([np.tile(B, (64, 1)), np.tile(A, (64, 1)), np.tile(Dd, (64, 1))])
    return MG.clusters(302, cs, ct, D)


def test_skipped_tiles_and_the_non_finite_flag(pkg, greg):
    sc = _skip_scene()
    prob, got = _check(pkg, greg, sc, MG.GATE, what="skipped tiles")
    blocks = prob.adm.reshape(3, 128, 3, 64).any(axis=(1, 3))
    assert blocks.tolist() == [[False, True, False], [True, False, False], [False, False, False]]
    assert not prob.adm[256:].any() and not prob.adm[:, 128:].any() and got[(("knn", 1),)]["n"] > 100
    # a non-finite value where every tile that would stage it is skipped: the flag depends on the input alone
    cases = []
    for val in (np.nan, np.inf):
        cases += [("fsrc", (300, 7), val), ("ftgt", (150, 32), val), ("src_pts", (300, 1), val), ("tgt_pts", (150, 2), val)]
    cases += [("fsrc", (383, 32), -np.inf), ("tgt_pts", (191, 0), np.nan)]
    for which, pos, val in cases:
        bad = MG.Scene(sc.src_pts.copy(), sc.fsrc.copy(), sc.tgt_pts.copy(), sc.ftgt.copy(), sc.Rt)
        getattr(bad, which)[pos] = val
        for kw in (dict(knn=1), dict(knn=1, mutual=True)):
            cnt = _device(pkg, greg, bad, MG.GATE, **kw)[0]
            rc, n, text = _raw(pkg, greg, bad, MG.GATE, **kw)
            print(which, pos, val, kw, cnt, rc, n, text)
            assert cnt == (0, 1), (which, pos, val, kw)
            assert rc == SC_EINVAL and n == 0 and "non-finite" in text, (which, pos, val, kw)
    for k, val in ((0, np.nan), (5, np.inf), (11, np.nan), (10, -np.inf)):
        Rt = sc.Rt.copy(); Rt[k] = val
        assert _device(pkg, greg, sc, MG.GATE, Rt=Rt)[0] == (0, 1), (k, val)
        rc, n, text = _raw(pkg, greg, sc, MG.GATE, Rt=Rt, knn=3)
        assert rc == SC_EINVAL and n == 0 and "pose" in text, (k, val)
    with pytest.raises(pkg.SacCotError) as e:
        Rt = sc.Rt.copy(); Rt[3] = np.nan
        greg.match_guided(*sc.args()[:4], Rt, gate=MG.GATE)
    assert e.value.status == SC_EINVAL
    _check(pkg, greg, sc, MG.GATE, modes=[dict(knn=2)], what="the context is usable afterwards")


# ---- 4: the boundary of the gate ---------------------------------------------------------------------------------
def test_the_boundary_of_the_gate(pkg, greg):
    half = np.float32(0.5)
    below = np.nextafter(half, np.float32(0))
    ident = AR.rt_of(np.eye(3), np.zeros(3))
    sc = MG.Scene(np.zeros((1, 3), np.float32), np.zeros((1, 1), np.float32), np.array([[half, 0, 0], [below, 0, 0]], np.float32),
                  np.array([[0.0], [1.0]], np.float32), ident)
    prob, got = _check(pkg, greg, sc, 0.5, what="g2 == gate2 is not admissible")
    assert prob.g2[0, 0] == np.float32(0.25) == MG.gate2_of(0.5) and prob.g2[0, 1] < np.float32(0.25)
    assert prob.adm.tolist() == [[False, True]]
    # (the nearer descriptor sits at the inadmissible target: the blind match would be (0, 0))
    assert got[(("knn", 4),)]["corr"].tolist() == [[0, 1]] and got[(("knn", 1), ("ratio", 0.8))]["n"] == 1
    # a finite pose whose residuals are NaN or inf admits nothing and raises no flag
    big = MG.shared_scene(130, 129, 33)
    hostile = MG.Scene(big.src_pts, big.fsrc, big.tgt_pts, big.ftgt, AR.hostile())
    for gate in (MG.GATE, MG.GATE_ALL, 3e38):
        prob, got = _check(pkg, greg, hostile, gate, modes=[dict(knn=4), dict(knn=1, mutual=True)], what="a hostile pose")
        assert not np.isfinite(prob.g2).any() and all(g["n"] == 0 for g in got.values())
        assert _device(pkg, greg, hostile, gate)[0] == (0, 0)


# ---- 5: a gate that admits everything is sc_match ----------------------------------------------------------------
def test_an_open_gate_equals_the_plain_match(pkg, greg):
    sc = MG.shared_scene(300, 333, 33)
    for kw in MODES:
        guided = greg.match_guided(*sc.args(), gate=MG.GATE_ALL, **kw)
        plain = greg.match(sc.fsrc, sc.ftgt, **kw)
        assert guided["n"] == plain["n"] > 0, kw
        assert guided["corr"].tobytes() == plain["corr"].tobytes() and guided["d2"].tobytes() == plain["d2"].tobytes(), kw


# ---- 6: forms and contexts agree ---------------------------------------------------------------------------------
def test_forms_and_contexts_agree(pkg, greg):
    sc = MG.shared_scene(300, 333, 33)
    for kw in (dict(knn=1), dict(knn=4), dict(knn=1, mutual=True), dict(knn=1, ratio=0.8), dict(knn=1, mutual=True, ratio=0.9)):
        host = greg.match_guided(*sc.args(), gate=MG.GATE, **kw)
        _same(host, MG.match(*sc.args(), MG.GATE, **kw), ("host form", kw))
        again = greg.match_guided(*sc.args(), gate=MG.GATE, **kw)
        fresh = pkg.Registrar(0)
        try:
            other = fresh.match_guided(*sc.args(), gate=MG.GATE, **kw)
            cnt, corr, d2, g2 = _device(pkg, fresh, sc, MG.GATE, pose_by_copy=True, **kw)
            cnt0, corr0, d20, _ = _device(pkg, fresh, sc, MG.GATE, want_g2=False, **kw)
        finally:
            fresh.close()
        assert cnt == cnt0 == (host["n"], 0), kw
        for x in (again, other, dict(corr=corr, d2=d2, g2=g2), dict(corr=corr0, d2=d20, g2=host["g2"])):
            assert x["corr"].tobytes() == host["corr"].tobytes() and x["d2"].tobytes() == host["d2"].tobytes(), kw
            assert x["g2"].tobytes() == host["g2"].tobytes(), kw


# ---- 7: descriptors and a prior in, (R, t), correspondences and mask out -----------------------------------------
def _flat(res):
    return np.concatenate([res["R"].ravel(), res["t"]])


def test_register_guided_features_equals_the_composition(pkg):
    S = pkg.synth
    cfg = S.CONFIGS["C0"]
    sc = S.make_feature_scene(cfg, 300, 32, 1.0)
    kw = cfg.params()
    p = pkg.make_params(**kw)
    gate = 3 * cfg.tau
    prior = AR.perturbed(AR.rt_of(sc.R_gt, sc.t_gt), 1, 17, angle=0.05, shift=cfg.tau / 2)[0]  # a few degrees off the true pose
    assert 1.0 < S.rotation_error_deg(prior[:9].reshape(3, 3), sc.R_gt) < 10.0
    prob = MG.Problem(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, prior, gate)
    r, r2 = pkg.Registrar(0), pkg.Registrar(0)
    try:
        for mode in (dict(), dict(mutual=True), dict(ratio=0.9)):
            exp = prob.match(knn=1, **mode)
            got = r.register_guided_features(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, prior, gate=gate, params=p, **mode)
            _same(got, exp, ("register_guided_features", mode))
            match = r2.match_guided(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, prior, gate=gate, **mode)
            assert match["corr"].tobytes() == got["corr"].tobytes()
            src = np.ascontiguousarray(sc.src_pts[match["corr"][:, 0]]); tgt = np.ascontiguousarray(sc.tgt_pts[match["corr"][:, 1]])
            plain = r2.register(src, tgt, params=p)
            kept_true = int((sc.truth[exp[0][:, 0]] == exp[0][:, 1]).sum())
            print(mode, "n", got["n"], "true pairs kept", kept_true, "of", int((sc.truth >= 0).sum()), "status", got["status"], "winner",
                  got["stats"]["best_count"])
            assert got["n"] >= 3 and kept_true > 0
            assert plain["status"] == got["status"] == SC_OK and np.array_equal(plain["mask"], got["mask"]), mode
            assert nan_equal_bits(_flat(plain), _flat(got)), mode
            for k in ("n", "edges", "tri_total", "tri_kept", "tri_scored", "best_rank", "best_count"):
                assert plain["stats"][k] == got["stats"][k], (mode, k)
            x, y = r.peel(), r2.peel()  # the call leaves that frame: a round on the matched correspondences is accepted
            assert x["status"] == y["status"] and np.array_equal(x["mask"], y["mask"]) and nan_equal_bits(_flat(x), _flat(y)), mode
            assert len(x["mask"]) == got["n"]
        # SoA keypoints give the same answer
        soa = r.register_guided_features(np.ascontiguousarray(sc.src_pts.T), sc.fsrc, np.ascontiguousarray(sc.tgt_pts.T), sc.ftgt, prior,
                                         gate=gate, ratio=0.9, layout=pkg.SC_SOA, **kw)
        assert soa["corr"].tobytes() == got["corr"].tobytes() and np.array_equal(soa["mask"], got["mask"]) and nan_equal_bits(_flat(soa), _flat(got))
        # fewer than three matches: SC_ENOHYP, R = I, the matches still returned; no frame is left
        two = r.register_guided_features(sc.src_pts[:2], sc.fsrc[:2], sc.tgt_pts, sc.ftgt, prior, gate=gate, params=p)
        exp = MG.match(sc.src_pts[:2], sc.fsrc[:2], sc.tgt_pts, sc.ftgt, prior, gate)
        assert two["status"] == SC_ENOHYP and two["n"] == len(exp[0]) < 3 and np.array_equal(two["corr"], exp[0])
        assert np.array_equal(two["R"], np.eye(3, dtype=np.float32)) and not two["t"].any()
        with pytest.raises(pkg.SacCotError) as e:
            r.peel()
        assert e.value.status == SC_EINVAL
    finally:
        r.close(); r2.close()


# ---- 8: refusals reach the C entries -----------------------------------------------------------------------------
def test_refusals_name_the_field(pkg):
    import torch
    sc = MG.shared_scene(65, 63, 33)
    G, M = pkg.make_guide_params, pkg.api.make_match_params
    r = pkg.Registrar(0)
    try:
        good = r.match_guided(*sc.args(), gate=MG.GATE)
        wrong_size = G(0.1); wrong_size.size = 28
        reserved = G(0.1); reserved.reserved[2] = 1
        for g, word in ((G(0.0), "gate"), (G(-1.0), "gate"), (G(float("nan")), "gate"), (G(float("inf")), "gate"), (G(0.1, 2), "layout"),
                        (G(0.1, 0, 1), "flags"), (wrong_size, "size"), (reserved, "reserved")):
            with pytest.raises(pkg.SacCotError) as e:
                r.match_guided(*sc.args(), gparams=g)
            assert e.value.status == SC_EINVAL and word in str(e.value) and "sc_match_guided" in str(e.value), word
        with pytest.raises(pkg.SacCotError) as e:  # every rule of sc_match_params
            r.match_guided(*sc.args(), gate=0.1, mparams=M(33, knn=2, mutual=True))
        assert e.value.status == SC_EINVAL and "knn == 1" in str(e.value)
        # the device entry: a NULL d_corr, then a call outstanding on the context
        dev = torch.device("cuda:0")
        d = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev) for x in sc.args()]
        d_corr = torch.zeros((65, 2), dtype=torch.int32, device=dev); d_d2 = torch.zeros(65, dtype=torch.float32, device=dev)
        d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def call(corr_ptr, g=G(0.1)):
            r.match_guided_device(d[0].data_ptr(), d[1].data_ptr(), 65, d[2].data_ptr(), d[3].data_ptr(), 63, M(33), g, d[4].data_ptr(),
                                  corr_ptr, d_d2.data_ptr(), None, d_cnt.data_ptr())

        with pytest.raises(pkg.SacCotError) as e:
            call(None)
        assert e.value.status == SC_EINVAL and "d_corr" in str(e.value)
        with pytest.raises(pkg.SacCotError) as e:
            call(d_corr.data_ptr(), G(0.1, 7))
        assert e.value.status == SC_EINVAL and "layout" in str(e.value)
        S = pkg.synth
        _, c0 = S.make_config_scene("C0")
        ds, dt = torch.from_numpy(c0.src).to(dev), torch.from_numpy(c0.tgt).to(dev)
        d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(len(c0.src), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        r.register_device_async(ds.data_ptr(), dt.data_ptr(), len(c0.src), pkg.make_params(**S.CONFIGS["C0"].params()), d_Rt.data_ptr(),
                                d_mask.data_ptr())
        with pytest.raises(pkg.SacCotError) as e:
            call(d_corr.data_ptr())
        assert e.value.status == SC_EINVAL and "outstanding" in str(e.value)
        r.wait()
        # nothing was enqueued by a refused call, and the context is as good as before
        again = r.match_guided(*sc.args(), gate=MG.GATE)
        assert again["corr"].tobytes() == good["corr"].tobytes() and again["g2"].tobytes() == good["g2"].tobytes()
    finally:
        r.close()
