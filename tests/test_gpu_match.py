"""GPU: descriptor matching (include/saccot.h, sc_match / sc_match_device / sc_register_features).

Every comparison is bit for bit against the numpy restatement of the canonical matcher (tests/match_ref.py): the
correspondences, the bits of the squared distances, the count.  sc_register_features is compared with the composition
restatement -> oracle register, and with sc_register on the same correspondences.
"""
import ctypes as C

import numpy as np
import pytest

import match_ref
from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
MODES = [dict(knn=1), dict(knn=2), dict(knn=3), dict(knn=4), dict(knn=1, mutual=True), dict(knn=1, ratio=0.8), dict(knn=1, ratio=0.9999)]
SHAPES = [(1, 1), (3, 5), (64, 64), (65, 63), (500, 777), (2000, 2300), (5000, 5300)]
DIMS = [1, 3, 32, 33, 352, 1024]


@pytest.fixture(scope="module")
def mreg(pkg):
    r = pkg.Registrar(0)
    yield r
    r.close()


def _descriptors(seed, ns, nt, D, sd=0.3):
    """Gaussian descriptors; the first third of the target rows are noisy copies of source rows (so the ratio test keeps some)."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((ns, D)).astype(np.float32)
    b = rng.standard_normal((nt, D)).astype(np.float32)
    m = min(ns, nt) // 3
    if m:
        rows = rng.permutation(nt)[:m]
        b[rows] = a[rng.permutation(ns)[:m]] + np.float32(sd) * rng.standard_normal((m, D)).astype(np.float32)
    return a, b


def _check(r, a, b, modes=MODES, what=""):
    acc = match_ref.distances(a, b)
    order, back = match_ref.ranked(acc)
    out = {}
    for kw in modes:
        exp_c, exp_d = match_ref.select(acc, order, back, **kw)
        got = r.match(a, b, **kw)
        tag = (what, a.shape, b.shape, kw)
        print(tag, "n", got["n"], "expected", len(exp_c))
        assert got["n"] == len(exp_c), tag
        assert np.array_equal(got["corr"], exp_c), tag
        assert got["d2"].view(np.uint32).tobytes() == exp_d.view(np.uint32).tobytes(), tag
        out[tuple(sorted(kw.items()))] = got
    return out


# ---- 1: shapes x descriptor lengths x modes ----------------------------------------------------------------------
# (the two large shapes at D <= 33 only: the restatement's time)
CASES = [(ns, nt, D) for (ns, nt) in SHAPES for D in DIMS if ns < 2000 or D <= 33]


@pytest.mark.parametrize("ns,nt,D", CASES)
def test_match_equals_the_restatement(mreg, ns, nt, D):
    a, b = _descriptors(1000 * D + ns, ns, nt, D)
    got = _check(mreg, a, b)
    if nt < 4:  # fewer targets than neighbours asked for: every row yields nt
        assert got[(("knn", 4),)]["n"] == ns * nt
    if ns >= 64 and D >= 32:  # the tests discriminate: something is dropped, something is kept
        for key in ((("knn", 1), ("mutual", True)), (("knn", 1), ("ratio", 0.8))):
            assert 0 < got[key]["n"] < ns, key


# ---- 2: planted ties ----------------------------------------------------------------------------------------------
def test_planted_ties(mreg):
    a, b = _descriptors(5, 200, 260, 33)
    b[7] = b[200]; b[130] = b[200]; b[201] = b[200]      # a target row four times
    a[150] = a[3]; a[199] = a[3]; a[64] = a[3]           # a source row four times
    b[40] = a[3]                                         # ... with an exact match
    _check(mreg, a, b, what="duplicates")
    # all-equal descriptors: every distance 0, the answer is pure index order
    one = np.full((130, 5), 0.75, np.float32)
    got = _check(mreg, one, np.full((70, 5), 0.75, np.float32), what="all equal")
    assert got[(("knn", 4),)]["corr"][:5].tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [1, 0]]
    assert got[(("knn", 1), ("mutual", True))]["corr"].tolist() == [[0, 0]]
    # two targets whose distances differ in the last bit, the nearer one at the higher index
    a2 = np.zeros((1, 2), np.float32)
    b2 = np.array([[1, np.float32(2.0 ** -11.5)], [1, 0], [1, np.float32(2.0 ** -11.5)]], np.float32)
    d = match_ref.distances(a2, b2).view(np.uint32)[0]
    assert int(d[0]) - int(d[1]) == 1 and d[0] == d[2]
    got = _check(mreg, a2, b2, what="last bit")
    assert got[(("knn", 3),)]["corr"][:, 1].tolist() == [1, 0, 2]


# ---- 3: magnitudes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-70, -20, 20, 60])
def test_magnitudes(mreg, k):
    a, b = _descriptors(11, 65, 63, 33)
    s = np.float32(2.0 ** k)
    acc = match_ref.distances(a * s, b * s)
    if k == -70:
        assert (acc == 0).all() or (acc[acc > 0] < 1e-38).all()   # the squares underflow: zeros and subnormals
    _check(mreg, a * s, b * s, what=f"2^{k}")
    a, b = _descriptors(12, 130, 129, 352)
    if k == 60:  # 352 squares of ~2^121 overflow to +inf, the planted near copies stay finite: still ordered, by bits then index
        acc = match_ref.distances(a * s, b * s)
        assert np.isinf(acc).any() and np.isfinite(acc).any()
    _check(mreg, a * s, b * s, modes=[dict(knn=4), dict(knn=1, mutual=True), dict(knn=1, ratio=0.9999)], what=f"2^{k} D 352")


# ---- 4: refusals --------------------------------------------------------------------------------------------------
def test_non_finite_descriptors_are_refused(pkg, mreg):
    import torch
    a, b = _descriptors(21, 300, 310, 33)
    for which, pos, val in (("src", (0, 0), np.inf), ("tgt", (309, 32), np.nan), ("src", (299, 32), -np.inf), ("tgt", (128, 16), np.nan)):
        a2, b2 = a.copy(), b.copy()
        (a2 if which == "src" else b2)[pos] = val
        for kw in (dict(knn=1), dict(knn=3), dict(knn=1, mutual=True)):
            with pytest.raises(pkg.SacCotError) as e:
                mreg.match(a2, b2, **kw)
            assert e.value.status == SC_EINVAL
        # the device entry reports it in stream order: count 0, flag 1
        dev = torch.device("cuda:0")
        da, db = torch.from_numpy(a2).to(dev), torch.from_numpy(b2).to(dev)
        d_corr = torch.zeros((300, 2), dtype=torch.int32, device=dev); d_d2 = torch.zeros(300, dtype=torch.float32, device=dev)
        d_cnt = torch.full((2,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()  # (the context's private stream is ordered against nothing)
        mreg.match_device(da.data_ptr(), 300, db.data_ptr(), 310, pkg.api.make_match_params(33), d_corr.data_ptr(), d_d2.data_ptr(), d_cnt.data_ptr())
        mreg.set_stream(None)  # (synchronises the context's stream)
        assert d_cnt.cpu().tolist() == [0, 1]
    _check(mreg, a, b, what="the context is usable afterwards")
    sc = pkg.synth.make_feature_scene(pkg.synth.CONFIGS["C0"], 300, 32, 1.0)
    f = sc.fsrc.copy(); f[17, 5] = np.nan
    with pytest.raises(pkg.SacCotError) as e:
        mreg.register_features(sc.src_pts, f, sc.tgt_pts, sc.ftgt, **pkg.synth.CONFIGS["C0"].params())
    assert e.value.status == SC_EINVAL


def test_bad_parameters_are_refused(pkg, mreg):
    a, b = _descriptors(22, 10, 12, 8)
    M = pkg.api.make_match_params
    bad = [M(8, knn=0), M(8, knn=5), M(8, knn=2, mutual=True), M(8, knn=2, ratio=0.5), M(0), M(1025), M(8, ratio=1.0), M(8, ratio=-0.5),
           M(8, ratio=float("nan")), M(8, flags=2)]
    wrong_size = M(8); wrong_size.size = C.sizeof(pkg.api.ScMatchParams) - 4
    reserved = M(8); reserved.reserved[1] = 1
    for m in bad + [wrong_size, reserved]:
        with pytest.raises(pkg.SacCotError) as e:
            mreg.match(a, b, mparams=m)
        assert e.value.status == SC_EINVAL, (m.dim, m.knn, m.flags, m.ratio)
    L = pkg.load_library()
    assert L.sc_match(mreg._h, None, 10, None, 12, C.byref(M(8)), None, None, None) == SC_EINVAL
    _check(mreg, a, b, modes=[dict(knn=2)], what="usable afterwards")


# ---- 5: entries and contexts agree --------------------------------------------------------------------------------
def test_host_entry_equals_device_entry_and_contexts_agree(pkg, mreg):
    import torch
    dev = torch.device("cuda:0")
    a, b = _descriptors(31, 700, 901, 33)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    for kw in (dict(knn=1), dict(knn=4), dict(knn=1, mutual=True), dict(knn=1, ratio=0.8), dict(knn=1, mutual=True, ratio=0.9)):
        host = mreg.match(a, b, **kw)
        exp_c, exp_d = match_ref.match(a, b, **kw)
        assert np.array_equal(host["corr"], exp_c) and host["d2"].tobytes() == exp_d.tobytes(), kw
        again = mreg.match(a, b, **kw)
        fresh = pkg.Registrar(0)
        try:
            other = fresh.match(a, b, **kw)
            cap = 700 * kw["knn"]
            d_corr = torch.full((cap, 2), -1, dtype=torch.int32, device=dev); d_d2 = torch.zeros(cap, dtype=torch.float32, device=dev)
            d_cnt = torch.full((2,), 7, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            fresh.set_stream(torch.cuda.current_stream().cuda_stream)
            fresh.match_device(da.data_ptr(), 700, db.data_ptr(), 901, pkg.api.make_match_params(33, **kw), d_corr.data_ptr(),
                               d_d2.data_ptr(), d_cnt.data_ptr())
            torch.cuda.synchronize()
        finally:
            fresh.close()
        n, flag = d_cnt.cpu().tolist()
        assert (n, flag) == (host["n"], 0), kw
        for x in (again, other, dict(corr=d_corr.cpu().numpy()[:n], d2=d_d2.cpu().numpy()[:n])):
            assert x["corr"].tobytes() == host["corr"].tobytes() and x["d2"].tobytes() == host["d2"].tobytes(), kw
        assert (d_corr.cpu().numpy()[n:] == -1).all()  # nothing is written behind the count


# ---- 6: descriptors in, (R, t), correspondences and mask out ------------------------------------------------------
def _flat(res):
    return np.concatenate([res["R"].ravel(), res["t"]])


@pytest.mark.parametrize("name,D", [("C0", 32), ("C1", 32), ("C2", 33)])
def test_register_features_equals_the_composition(pkg, O, name, D):
    S = pkg.synth
    cfg = S.CONFIGS[name]
    sc = S.make_feature_scene(cfg, 300, D, 1.0)
    kw = cfg.params()
    p = pkg.make_params(**kw)
    acc = match_ref.distances(sc.fsrc, sc.ftgt)
    order, back = match_ref.ranked(acc)
    threads = min(O.max_threads(), 16)
    r, r2 = pkg.Registrar(0), pkg.Registrar(0)
    try:
        ws = []
        for mode in (dict(), dict(mutual=True), dict(ratio=0.9)):
            exp_c, exp_d = match_ref.select(acc, order, back, knn=1, **mode)
            got = r.register_features(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, params=p, **mode)
            ws.append(got["stats"]["workspace_bytes"])
            tag = (name, mode)
            assert got["n"] == len(exp_c) and np.array_equal(got["corr"], exp_c) and got["d2"].tobytes() == exp_d.tobytes(), tag
            src, tgt = np.ascontiguousarray(sc.src_pts[exp_c[:, 0]]), np.ascontiguousarray(sc.tgt_pts[exp_c[:, 1]])
            ref = O.register(src, tgt, threads=threads, **kw)
            plain = r2.register(src, tgt, params=p)
            kept_true = int((sc.truth[exp_c[:, 0]] == exp_c[:, 1]).sum())
            terr = float(np.linalg.norm(ref["t"].astype(np.float64) - sc.t_gt))
            print(tag, "n", got["n"], "true pairs kept", kept_true, "of", int((sc.truth >= 0).sum()), "status", got["status"], "winner",
                  got["stats"]["best_count"], "rank", got["stats"]["best_rank"], "| oracle", ref["rc"], ref["best_count"], ref["best_rank"],
                  "t err / tau %.3f" % (terr / cfg.tau), "rot err %.3f deg" % S.rotation_error_deg(ref["R"], sc.R_gt))
            # meaning, on the reference (and so, by the equalities below, on the GPU)
            assert ref["rc"] == SC_OK and ref["best_count"] >= 0.85 * kept_true and terr < cfg.tau, tag
            # ... the oracle composition, bit for bit
            assert got["status"] == ref["rc"], tag
            assert got["stats"]["best_count"] == ref["best_count"] and got["stats"]["best_rank"] == ref["best_rank"], tag
            assert np.array_equal(got["mask"], ref["mask"]), tag
            assert nan_equal_bits(_flat(got), _flat(ref)), tag
            # ... and sc_register on those correspondences
            assert plain["status"] == got["status"] and np.array_equal(plain["mask"], got["mask"]) and nan_equal_bits(_flat(plain), _flat(got)), tag
            for k in ("n", "edges", "tri_total", "tri_kept", "tri_scored", "best_rank", "best_count"):
                assert plain["stats"][k] == got["stats"][k], (tag, k)
            # the call leaves a frame: rounds on the matched correspondences
            for rnd in range(2):
                x, y = r.peel(), r2.peel()
                assert x["status"] == y["status"] and np.array_equal(x["mask"], y["mask"]) and nan_equal_bits(_flat(x), _flat(y)), (tag, rnd)
                assert x["stats"]["best_count"] == y["stats"]["best_count"] and len(x["mask"]) == got["n"], (tag, rnd)
        again = r.register_features(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, params=p)
        assert again["corr"].tobytes() == match_ref.select(acc, order, back)[0].tobytes() and again["stats"]["workspace_bytes"] >= ws[0] > 0
    finally:
        r.close(); r2.close()


def test_register_features_small_and_layouts(pkg, mreg):
    S = pkg.synth
    cfg = S.CONFIGS["C0"]
    sc = S.make_feature_scene(cfg, 300, 32, 1.0)
    kw = cfg.params()
    # SoA points give the same answer as AoS points
    aos = mreg.register_features(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, mutual=True, **kw)
    soa = mreg.register_features(np.ascontiguousarray(sc.src_pts.T), sc.fsrc, np.ascontiguousarray(sc.tgt_pts.T), sc.ftgt, mutual=True,
                                 layout=pkg.SC_SOA, **kw)
    assert aos["status"] == soa["status"] == SC_OK and aos["corr"].tobytes() == soa["corr"].tobytes()
    assert np.array_equal(aos["mask"], soa["mask"]) and nan_equal_bits(_flat(aos), _flat(soa))
    # a repeated shape allocates nothing: the matcher's workspace grows once, in the first call of the shape.  workspace_bytes is
    # read through a small registration that has settled first (the registration sizes its own buffers by its history, and with
    # the host-free enqueue off the same input takes the same path every time), so whatever moves afterwards is the matcher's.
    r = pkg.Registrar(0)
    try:
        r.set_debug(no_fast=1)
        _, c0 = S.make_config_scene("C0")
        probe = [r.register(c0.src, c0.tgt, **kw)["stats"]["workspace_bytes"] for _ in range(4)]
        assert probe[2] == probe[3] > 0, probe
        a, b = _descriptors(41, 3000, 3100, 33)
        r.match(a, b, mutual=True)
        w1 = r.register(c0.src, c0.tgt, **kw)["stats"]["workspace_bytes"]
        for _ in range(2):
            r.match(a, b, mutual=True)
        w2 = r.register(c0.src, c0.tgt, **kw)["stats"]["workspace_bytes"]
        print("workspace bytes: settled", probe, "after the first match", w1, "after three", w2)
        assert w1 > probe[3] and w2 == w1
    finally:
        r.close()
    # fewer than three matches: SC_ENOHYP, R = I, the matches still returned; no frame is left
    two = mreg.register_features(sc.src_pts[:2], sc.fsrc[:2], sc.tgt_pts, sc.ftgt, **kw)
    exp_c, exp_d = match_ref.match(sc.fsrc[:2], sc.ftgt)
    assert two["status"] == SC_ENOHYP and two["n"] == 2 and np.array_equal(two["corr"], exp_c) and two["d2"].tobytes() == exp_d.tobytes()
    assert np.array_equal(two["R"], np.eye(3, dtype=np.float32)) and not two["t"].any()
    with pytest.raises(pkg.SacCotError) as e:
        mreg.peel()
    assert e.value.status == SC_EINVAL
    # sc_match ends a frame like every other computing entry
    mreg.register_features(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, **kw)
    mreg.match(sc.fsrc[:5], sc.ftgt[:9])
    with pytest.raises(pkg.SacCotError) as e:
        mreg.peel()
    assert e.value.status == SC_EINVAL
