"""GPU parity: every stage of the HIP path, called through the C ABI (libsaccot.so), must equal the CPU
restatement (oracle/saccot_oracle.c) BIT FOR BIT on the same seeded inputs — adjacency bits, degrees, weights,
the ranked triangle list (order included), every (R,t), every inlier count, the winner and the mask.

PARITY UNPINNED: the reference (/root/reference/README.md:1-2) has no implementation or vectors; the oracle is this
repo's restatement of SURVEY.md §8(a), itself cross-checked against an fp64 numpy restatement in the CPU suite.
"""
import numpy as np
import pytest

from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu


def _scene(pkg, n, rho=0.3, L=1.0, tau=0.05, seed=7):
    return pkg.synth.make_scene(n, rho, L, tau, seed)


def _params(pkg, tau, T, **kw):
    d = dict(sigma=tau, t_cmp=0.9, tau=tau, min_len=tau, max_triangles=T, rank_mode=0)
    d.update(kw)
    return d


# ---------------------------------------------------------------------------------------------------------
# stage A
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(3, 1), (64, 2), (65, 3), (500, 1000), (777, 4), (1024, 5), (2000, 1001)])
def test_compat_bit_exact(pkg, O, reg, n, seed):
    sc = _scene(pkg, n, seed=seed)
    kw = _params(pkg, 0.05, 10)
    S, bits, deg = reg.compat(sc.src, sc.tgt, pkg.make_params(**kw))
    S0, bits0, deg0 = O.compat(sc.src, sc.tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"])
    assert np.array_equal(bits, bits0)
    assert np.array_equal(deg, deg0)
    assert np.array_equal(S.view(np.uint32), S0.view(np.uint32))
    assert np.array_equal(S, S.T) and not S.diagonal().any()


@pytest.mark.parametrize("one_phase,rows", [(False, "16"), (True, "16"), (False, "32"), (True, "32"), (False, "64")])
@pytest.mark.parametrize("min_len_scale", [0.0, 1.0])
def test_compat_both_interior_forms_bit_exact(pkg, O, one_phase, rows, min_len_scale):
    """Interior tiles of stage A run a conservative candidate test on squared lengths and the exact chain only on the
    candidates (default), or the exact chain on every pair (sc_debug.compat_one_phase): both against the CPU restatement,
    with min_len = 0 (coincident-point candidates) and on a scene with exact duplicates and near-threshold pairs."""
    sc = pkg.synth.make_scene(1500, 0.3, 1.0, 0.05, seed=77)
    src, tgt = sc.src.copy(), sc.tgt.copy()
    src[100:164] = src[36:100]; tgt[100:164] = tgt[36:100]        # exact duplicates: zero lengths, ties
    tgt[200:400] = src[200:400] * np.float32(1.0) + np.float32(0.25)  # a pure translation block: d == 0 exactly
    kw = dict(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05 * min_len_scale)
    r = pkg.Registrar(0)
    try:
        r.set_debug(compat_one_phase=int(one_phase), compat_rows=int(rows))  # 32-row tiles: the default from 10 000 correspondences; 64: experimental
        S1, b1, d1 = r.compat(src, tgt, pkg.make_params(**kw))
    finally:
        r.close()
    S0, b0, d0 = O.compat(src, tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"])
    assert np.array_equal(b1, b0) and np.array_equal(d1, d0)
    assert np.array_equal(S1.view(np.uint32), S0.view(np.uint32))


@pytest.mark.parametrize("one_phase", [False, True])
@pytest.mark.parametrize("eps,scale", [(0.03, 1.0), (0.002, 40.0), (0.25, 0.01)])
def test_compat_threshold_sweep_on_a_scaled_scene(pkg, O, eps, scale, one_phase):
    """q = (1 + eps) p: the rigidity residual d = eps * |p_i - p_j| sweeps continuously through d_thr, so of the ~1.1 M
    pairs many sit within a few ulps of the threshold (and of min_len) — where the candidate test of the two-phase
    interior tiles has to err on the safe side.  Bit-exact S, bit rows and degrees against the CPU restatement."""
    rng = np.random.default_rng(7)
    src = (rng.random((1500, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(scale)
    tgt = (src * np.float32(1.0 + eps)).astype(np.float32)
    typical = 0.66 * scale                       # mean distance of two uniform points in a cube of this edge
    sigma = eps * typical / 0.459                # d_thr = 0.459 sigma at t_cmp = 0.9  ->  threshold mid-range
    kw = dict(sigma=sigma, t_cmp=0.9, tau=sigma, min_len=0.3 * scale)
    r = pkg.Registrar(0)
    try:
        r.set_debug(compat_one_phase=int(one_phase))
        S1, b1, d1 = r.compat(src, tgt, pkg.make_params(**kw))
    finally:
        r.close()
    S0, b0, d0 = O.compat(src, tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"])
    assert 0.05 < d0.mean() / 1500 < 0.9          # the threshold really cuts through the distribution
    assert np.array_equal(b1, b0) and np.array_equal(d1, d0)
    assert np.array_equal(S1.view(np.uint32), S0.view(np.uint32))


@pytest.mark.parametrize("mode", [0, 1, 4, 3, 6])
def test_compat_store_forms_bit_exact(pkg, O, mode):
    """Stage A writes S with 4-byte or 16-byte stores depending on the matrix size; sc_debug.compat_store_mode forces
    either form (bit 0 / bit 2) and adds the non-temporal hint (bit 1).  Same bits in S, the bit rows and the degrees
    in every form, ragged N."""
    sc = pkg.synth.make_scene(1337, 0.3, 1.0, 0.05, seed=5)
    kw = _params(pkg, 0.05, 10)
    r = pkg.Registrar(0)
    try:
        r.set_debug(compat_store_mode=mode)
        S, bits, deg = r.compat(sc.src, sc.tgt, pkg.make_params(**kw))
    finally:
        r.close()
    S0, bits0, deg0 = O.compat(sc.src, sc.tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"])
    assert np.array_equal(bits, bits0) and np.array_equal(deg, deg0)
    assert np.array_equal(S.view(np.uint32), S0.view(np.uint32))


@pytest.mark.parametrize("name", ["C0", "C1", "C2"])
def test_no_dense_S_changes_nothing(pkg, O, reg, name):
    """SC_FLAG_NO_DENSE_S: stage A writes the adjacency bit rows only.  Nothing after stage A reads S (edge weights are
    recomputed from the points with the same chain), so the bit rows, degrees and the whole result equal the
    restatement's exactly as with the dense matrix; asking the stage hook for S together with the flag is an error."""
    cfg, scene = pkg.synth.make_config_scene(name)
    kw = cfg.params()
    _, bits, deg = reg.compat(scene.src, scene.tgt, pkg.make_params(flags=pkg.SC_FLAG_NO_DENSE_S, **kw), want_S=False)
    _, bits0, deg0 = O.compat(scene.src, scene.tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"], threads=8, want_S=False)
    assert np.array_equal(bits, bits0) and np.array_equal(deg, deg0)
    got = reg.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_NO_DENSE_S | pkg.SC_FLAG_EXACT_TOTAL, **kw)
    ref = O.register(scene.src, scene.tgt, threads=8, **kw)
    assert got["status"] == ref["rc"] == 0
    assert (got["stats"]["edges"], got["stats"]["tri_total"], got["stats"]["best_rank"]) == (ref["edges"], ref["tri_total"], ref["best_rank"])
    assert np.array_equal(got["mask"], ref["mask"]) and nan_equal_bits(got["R"], ref["R"]) and nan_equal_bits(got["t"], ref["t"])
    with pytest.raises(pkg.SacCotError):
        reg.compat(scene.src, scene.tgt, pkg.make_params(flags=pkg.SC_FLAG_NO_DENSE_S, **kw), want_S=True)


def test_compat_soa_layout_and_min_len_zero(pkg, O, reg):
    sc = _scene(pkg, 300, seed=11)
    kw = _params(pkg, 0.05, 10, min_len=0.0)
    p = pkg.make_params(layout=pkg.SC_SOA, **kw)
    S, bits, deg = reg.compat(np.ascontiguousarray(sc.src.T), np.ascontiguousarray(sc.tgt.T), p)
    S0, bits0, deg0 = O.compat(sc.src, sc.tgt, kw["sigma"], kw["t_cmp"], 0.0, kw["tau"])
    assert np.array_equal(bits, bits0) and np.array_equal(deg, deg0)
    assert np.array_equal(S.view(np.uint32), S0.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------
# stage B
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T,rank_mode,seed", [(64, 50, 0, 2), (500, 200, 0, 1000), (500, 200, 1, 1000),
                                                (777, 5000, 0, 4), (2000, 10000, 0, 1001), (2000, 10000, 1, 1001),
                                                (500, 10_000_000, 0, 1000)])
def test_triangles_ranked_list_bit_exact(pkg, O, reg, n, T, rank_mode, seed):
    tau = 0.05 if n != 2000 else 0.02
    rho = 0.3 if n != 2000 else 0.2
    sc = _scene(pkg, n, rho=rho, tau=tau, seed=seed)
    kw = _params(pkg, tau, T, rank_mode=rank_mode)
    tri, key, total, edges = reg.triangles(sc.src, sc.tgt, pkg.make_params(**kw))
    S0, bits0, deg0 = O.compat(sc.src, sc.tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"])
    tri0, key0, total0 = O.triangles(S0, bits0, deg0, T, rank_mode)
    assert total == total0 and edges == int(deg0.sum()) // 2
    assert tri.shape == tri0.shape == (min(T, total0), 3)
    assert np.array_equal(key, key0)
    assert np.array_equal(tri, tri0)


def test_triangles_massive_ties(pkg, O, reg):
    """Noise-free all-inlier scene: every weight is (nearly) the same float, so the top-T is decided almost
    entirely by the lexicographic tie-break — the path the ordinal-indexed select exists for."""
    sc = pkg.synth.make_scene(150, 1.0, 1.0, 1e-7, 21)
    kw = _params(pkg, 0.05, 3000)
    tri, key, total, _ = reg.triangles(sc.src, sc.tgt, pkg.make_params(**kw))
    S0, bits0, deg0 = O.compat(sc.src, sc.tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"])
    tri0, key0, total0 = O.triangles(S0, bits0, deg0, 3000, 0)
    assert total == total0 and total0 > 100_000
    assert len(np.unique(key0)) < 50
    assert np.array_equal(key, key0) and np.array_equal(tri, tri0)


@pytest.mark.parametrize("n,T", [(40, 500), (40, 1_000_000), (64, 3000), (96, 20_000)])
def test_select_whose_window_is_one_key_before_its_last_round(pkg, O, reg, n, T):
    """r05: a select round only fills its histogram; the NEXT launch resolves it.  Degree ranking on a complete graph — every vertex
    has the same degree, so every key is the same value: the key range is ONE value (a window of zero bits), round 0 already comes
    down to k*, rounds 1 and 2 find the select done and add nothing, the compaction's counting kernel resolves a round that never
    ran.  The top-T is then the first T triangles in (i, j, k) order; T beyond the triangle count takes them all."""
    sc = pkg.synth.make_scene(n, 1.0, 1.0, 1e-7, 7)
    kw = _params(pkg, 0.05, T, rank_mode=1)
    tri, key, total, _ = reg.triangles(sc.src, sc.tgt, pkg.make_params(**kw))
    S0, bits0, deg0 = O.compat(sc.src, sc.tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"])
    tri0, key0, total0 = O.triangles(S0, bits0, deg0, T, 1)
    assert total == total0 and len(np.unique(key0)) == 1   # (n = 40: the graph is complete — total = n (n - 1) (n - 2) / 6 — and the key RANGE is one value)
    if n == 40:
        assert total0 == n * (n - 1) * (n - 2) // 6
    assert np.array_equal(key, key0) and np.array_equal(tri, tri0)
    out = reg.register(sc.src, sc.tgt, **kw)
    ref = O.register(sc.src, sc.tgt, threads=4, **kw)
    assert out["status"] == ref["rc"] == 0 and out["stats"]["best_rank"] == ref["best_rank"] and np.array_equal(out["mask"], ref["mask"])


def test_triangles_none(pkg, reg):
    """A scene with no compatible pair at all: zero edges, zero triangles, and the path reports SC_ENOHYP."""
    rng = np.random.default_rng(5)
    src = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    tgt = (src * 37.0).astype(np.float32)  # every distance scaled: no rigid pair
    kw = _params(pkg, 0.001, 100)
    tri, key, total, edges = reg.triangles(src, tgt, pkg.make_params(**kw))
    assert total == 0 and edges == 0 and tri.shape[0] == 0
    out = reg.register(src, tgt, **kw)
    assert out["status"] == pkg.SC_ENOHYP
    assert np.array_equal(out["R"], np.eye(3, dtype=np.float32)) and not out["t"].any() and not out["mask"].any()


# ---------------------------------------------------------------------------------------------------------
# stage C1
# ---------------------------------------------------------------------------------------------------------
def test_kabsch_bit_exact_random_and_degenerate(pkg, O, reg):
    sc = _scene(pkg, 400, seed=31)
    rng = np.random.default_rng(3)
    tri = np.sort(rng.integers(0, 400, (5000, 3)), axis=1).astype(np.uint32)
    tri[:50, 1] = tri[:50, 0]                       # duplicate vertex: rank-1 H
    src = sc.src.copy(); tgt = sc.tgt.copy()
    src[:3] = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)  # collinear triangle (0,1,2)
    tri[50] = (0, 1, 2)
    tgt[3:6] = tgt[3]                               # coincident target points: H = 0
    tri[51] = (3, 4, 5)
    p = pkg.make_params(**_params(pkg, 0.05, 10))
    Rt = reg.kabsch(src, tgt, p, tri)
    Rt0 = O.kabsch3(src, tgt, tri)
    assert nan_equal_bits(Rt, Rt0)
    good = np.isfinite(Rt0).all(axis=1)
    assert good.sum() > 4000
    R = Rt0[good, :9].reshape(-1, 3, 3).astype(np.float64)
    assert np.abs(np.linalg.det(R) - 1).max() < 1e-4  # proper rotations


# ---------------------------------------------------------------------------------------------------------
# stage C2 / C3
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", [(500, 200), (1000, 257), (2000, 10000), (1025, 3000), (513, 70)])
def test_score_counts_bit_exact(pkg, O, n, T):
    """the plain C2 kernel (lane = hypothesis, the points in LDS); ragged point chunks and hypothesis counts"""
    reg = pkg.Registrar(0)
    sc = _scene(pkg, n, seed=n)
    rng = np.random.default_rng(n)
    tri = np.sort(np.stack([rng.choice(n, 3, replace=False) for _ in range(T)]), axis=1).astype(np.uint32)
    inl = np.nonzero(sc.inlier)[0]
    tri[: T // 2] = np.sort(np.stack([rng.choice(inl, 3, replace=False) for _ in range(T // 2)]), axis=1)
    Rt0 = O.kabsch3(sc.src, sc.tgt, tri)
    Rt0[7, 4] = np.nan                                # non-finite hypothesis scores 0
    kw = _params(pkg, 0.05, T)
    cnt, key = reg.score(sc.src, sc.tgt, pkg.make_params(**kw), Rt0)
    cnt0 = O.score(sc.src, sc.tgt, Rt0, kw["tau"])
    assert cnt0.max() > 20 and cnt0[7] == 0
    assert np.array_equal(cnt, cnt0)
    assert key == O.best_key(cnt0)
    best = 0xFFFFFFFF - (key & 0xFFFFFFFF)
    m = reg.mask(sc.src, sc.tgt, pkg.make_params(**kw), Rt0[best])
    assert np.array_equal(m, O.mask(sc.src, sc.tgt, Rt0[best], kw["tau"])) and m.sum() == cnt0[best]
    Rt1 = Rt0.copy(); Rt1[3, 9] = np.inf; Rt1[9, 0] = -np.inf; Rt1[11, 5] = np.nan       # every kind of non-finite entry
    cnt1, _ = reg.score(sc.src, sc.tgt, pkg.make_params(**kw), Rt1)
    assert np.array_equal(cnt1, O.score(sc.src, sc.tgt, Rt1, kw["tau"])) and not cnt1[[3, 9, 11]].any()
    reg.close()


# ---------------------------------------------------------------------------------------------------------
# whole path
# ---------------------------------------------------------------------------------------------------------
def _check_register(pkg, O, reg, scene, kw, threads=8):
    got = reg.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_EXACT_TOTAL, **kw)
    ref = O.register(scene.src, scene.tgt, threads=threads, **kw)
    assert got["status"] == ref["rc"]
    st = got["stats"]
    assert (st["edges"], st["tri_total"], st["tri_kept"]) == (ref["edges"], ref["tri_total"], ref["t_eff"])
    assert (st["best_rank"], st["best_count"]) == (ref["best_rank"], ref["best_count"])
    assert np.array_equal(got["mask"], ref["mask"])                      # bit-exact mask   [north_star]
    assert nan_equal_bits(got["R"], ref["R"]) and nan_equal_bits(got["t"], ref["t"])  # stronger than 1e-5
    return got, ref


@pytest.mark.parametrize("name", ["C0", "C1", "C2"])
def test_register_matches_oracle(pkg, O, reg, name):
    cfg, scene = pkg.synth.make_config_scene(name)
    got, _ = _check_register(pkg, O, reg, scene, cfg.params())
    # known-answer: synthetic ground truth (3-point hypotheses are coarse; bounds are loose on purpose)
    assert pkg.synth.rotation_error_deg(got["R"], scene.R_gt) < 3.0
    assert np.linalg.norm(got["t"] - scene.t_gt) < 2 * cfg.tau + 0.05 * cfg.L
    m = got["mask"].astype(bool)
    assert (m & scene.inlier).sum() >= 0.9 * scene.inlier.sum()


@pytest.mark.parametrize("name", ["C0", "C1", "C2"])
def test_certified_pruning_changes_nothing_but_the_work(pkg, reg, name):
    """Stage B enumerates only the certified 'strong' subgraph by default (sc_tri_prune.hip 3b).  The ranked list — keys,
    triangles, order — and the whole result must be identical with the pruning switched off, while the number of
    enumerated 3-cliques must drop."""
    cfg, scene = pkg.synth.make_config_scene(name)
    kw = cfg.params()
    tri_a, key_a, total_a, edges_a = reg.triangles(scene.src, scene.tgt, pkg.make_params(**kw))
    tri_b, key_b, total_b, edges_b = reg.triangles(scene.src, scene.tgt, pkg.make_params(flags=pkg.SC_FLAG_NO_PRUNE, **kw))
    assert (total_a, edges_a) == (total_b, edges_b)           # the hook always reports the whole graph
    assert np.array_equal(key_a, key_b) and np.array_equal(tri_a, tri_b)
    a = reg.register(scene.src, scene.tgt, **kw)
    b = reg.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_NO_PRUNE, **kw)
    assert np.array_equal(a["mask"], b["mask"]) and a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes()
    assert a["stats"]["best_rank"] == b["stats"]["best_rank"] and a["stats"]["tri_kept"] == b["stats"]["tri_kept"]
    assert kw["max_triangles"] <= a["stats"]["tri_total"] < b["stats"]["tri_total"]   # pruned < whole graph
    if name == "C2":
        assert a["stats"]["tri_total"] < b["stats"]["tri_total"] // 5


@pytest.mark.parametrize("knobs", [dict(cnt_blocks=37, keys_blocks=53, sel_blocks=7, sample_edges=5000),
                                   dict(cnt_blocks=4096, keys_blocks=1, sel_blocks=1, sample_edges=1000000, tg_sample=32, sample_blocks=3, sample_mode=2),
                                   dict(sample_mode=2, sample_edges=700, tg_sample=8, compact_self_max=100000, scan_self_max=0),
                                   dict(rows_unfused=1, scan_self_max=0),   # round 1's separate row_stats + three-kernel scans
                                   dict(no_events=1, tg_count=4, tg_keys=64, sel_blocks=3, sample_mode=1),
                                   dict(sample_mode=1, sample_edges=5000, tg_sample=4, tg_events=32)])
def test_results_do_not_depend_on_grid_or_sample_size(pkg, O, knobs):
    """Stage B's launch geometry and the size of the pruning sample only change the amount of work (a looser or tighter
    certified bound, more or fewer workgroups) — never the result: odd values for every scheduling knob on C1 and C2,
    set through sc_set_debug (the library reads no environment variable)."""
    r = pkg.Registrar(0)
    try:
        r.set_debug(**knobs)
        for name in ("C1", "C2"):
            cfg, scene = pkg.synth.make_config_scene(name)
            kw = cfg.params()
            ref = O.register(scene.src, scene.tgt, threads=1, **kw)
            got = r.register(scene.src, scene.tgt, **kw)         # tri_total depends on the bound: not compared here
            assert got["status"] == ref["rc"] == 0
            assert (got["stats"]["edges"], got["stats"]["tri_kept"]) == (ref["edges"], ref["t_eff"])
            assert (got["stats"]["best_rank"], got["stats"]["best_count"]) == (ref["best_rank"], ref["best_count"])
            assert np.array_equal(got["mask"], ref["mask"])
            assert nan_equal_bits(got["R"], ref["R"]) and nan_equal_bits(got["t"], ref["t"])
    finally:
        r.close()


def test_large_input_fallbacks_forced_on_a_small_one(pkg, O):
    """Two paths only very large inputs reach — the three-kernel scan (beyond 16.7 M elements) and the scanned
    compaction offsets (beyond 4096 key tiles) — forced by their sc_debug knobs on C1 / C2 and checked like any other run."""
    r = pkg.Registrar(0)
    try:
        r.set_debug(scan_self_max=0, compact_self_max=0)
        for name in ("C1", "C2"):
            cfg, scene = pkg.synth.make_config_scene(name)
            _check_register(pkg, O, r, scene, cfg.params())
    finally:
        r.close()


def test_register_degree_ranking_and_small_T(pkg, O, reg):
    cfg, scene = pkg.synth.make_config_scene("C0")
    kw = cfg.params(); kw["rank_mode"] = 1; kw["max_triangles"] = 37
    _check_register(pkg, O, reg, scene, kw)


@pytest.mark.parametrize("t_cmp", [0.5, 0.66, 0.67, 0.97])
def test_register_select_window_both_forms(pkg, O, reg, t_cmp):
    """Stage B's select takes its key window a priori ([certified bound or 2.0, 3.0], two rounds) when every edge
    weight is provably >= 2/3, and from the measured key range (three rounds) otherwise: t_cmp on both sides of the
    switch, against the CPU restatement; also the triangle list itself, pruned, against the unpruned one."""
    cfg, scene = pkg.synth.make_config_scene("C1")
    kw = cfg.params(); kw["t_cmp"] = t_cmp; kw["max_triangles"] = 4000
    _check_register(pkg, O, reg, scene, kw)
    tri_a, key_a, _, _ = reg.triangles(scene.src, scene.tgt, pkg.make_params(**kw))
    tri_b, key_b, _, _ = reg.triangles(scene.src, scene.tgt, pkg.make_params(flags=pkg.SC_FLAG_NO_PRUNE, **kw))
    assert np.array_equal(key_a, key_b) and np.array_equal(tri_a, tri_b)


@pytest.mark.parametrize("seed", list(range(16)))
def test_register_random_configurations(pkg, O, reg, seed):
    """Randomised sweep of the whole path against the CPU restatement: ragged N, random inlier ratio and scale, random
    sigma / t_cmp / tau / min_len / T, both ranking modes, and one context reused across all of them (so the
    speculative launches run into buffers of other sizes)."""
    rng = np.random.default_rng(1234 + seed)
    n = int(rng.integers(40, 1800))
    rho = float(rng.uniform(0.05, 0.6))
    L = float(10.0 ** rng.uniform(-1, 2))
    tau = L * float(rng.uniform(0.01, 0.06))
    scene = pkg.synth.make_scene(n, rho, L, tau, seed=500 + seed)
    kw = dict(sigma=tau * float(rng.uniform(0.5, 2.0)), t_cmp=float(rng.uniform(0.45, 0.98)), tau=tau,
              min_len=tau * float(rng.choice([0.0, 0.5, 1.0, 3.0])), max_triangles=int(rng.integers(1, 30000)),
              rank_mode=int(rng.integers(0, 2)))
    ref = O.register(scene.src, scene.tgt, threads=1, **kw)
    got = reg.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_EXACT_TOTAL, **kw)
    assert got["status"] == ref["rc"], (kw, n)
    st = got["stats"]
    assert (st["edges"], st["tri_total"], st["tri_kept"]) == (ref["edges"], ref["tri_total"], ref["t_eff"]), (kw, n)
    assert (st["best_rank"], st["best_count"]) == (ref["best_rank"], ref["best_count"]), (kw, n)
    assert np.array_equal(got["mask"], ref["mask"])
    assert nan_equal_bits(got["R"], ref["R"]) and nan_equal_bits(got["t"], ref["t"])


def test_register_deterministic_and_context_reuse(pkg, reg):
    """Same context, interleaved problem sizes (workspace grows, never shrinks): byte-identical repeats."""
    cfg1, s1 = pkg.synth.make_config_scene("C1")
    cfg0, s0 = pkg.synth.make_config_scene("C0")
    a = reg.register(s1.src, s1.tgt, **cfg1.params())
    reg.register(s0.src, s0.tgt, **cfg0.params())
    b = reg.register(s1.src, s1.tgt, **cfg1.params())
    assert np.array_equal(a["mask"], b["mask"]) and a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes()
    assert a["stats"]["best_rank"] == b["stats"]["best_rank"]


def test_register_sharded_equals_unsharded(pkg, reg):
    """SURVEY §8e on one GPU: run the two-phase API once per (rank, world) with the same context, max-reduce the
    keys on the host, finalize — the winner, (R,t) and mask must equal the unsharded run for every world size."""
    import torch
    cfg, scene = pkg.synth.make_config_scene("C1")
    base = reg.register(scene.src, scene.tgt, **cfg.params())
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    d_key = torch.zeros(2, dtype=torch.int64, device=dev)
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(cfg.n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for world in (1, 2, 3, 8):
        keys, scored = [], 0
        for rank in range(world):
            p = pkg.make_params(shard_rank=rank, shard_world=world, shard_block=256, **cfg.params())
            st = reg.hypothesize_device(d_src.data_ptr(), d_tgt.data_ptr(), cfg.n, p, d_key.data_ptr())
            torch.cuda.synchronize()
            keys.append(tuple(int(x) for x in d_key.cpu())); scored += st["tri_scored"]
        assert scored == base["stats"]["tri_kept"]
        if world % 2:
            k0, k1 = pkg.shard.reduce_pairs(keys)           # what the two all-reduces compute
            d_key.copy_(torch.tensor([k0, k1], dtype=torch.int64)); torch.cuda.synchronize()
            rc, st = reg.finalize_device(d_key.data_ptr(), d_Rt.data_ptr(), d_mask.data_ptr())
        else:                                               # what ONE all-gather delivers: the reduction runs in the kernel
            d_all = torch.tensor([x for k in keys for x in k], dtype=torch.int64).to(dev); torch.cuda.synchronize()
            rc, st = reg.finalize_gathered_device(d_all.data_ptr(), world, d_Rt.data_ptr(), d_mask.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and st["best_rank"] == base["stats"]["best_rank"] and st["best_count"] == base["stats"]["best_count"]
        assert np.array_equal(d_mask.cpu().numpy(), base["mask"])
        assert d_Rt.cpu().numpy().tobytes() == np.concatenate([base["R"].ravel(), base["t"]]).tobytes()


def test_split_phase1_sharded_sample_equals_unsharded(pkg, reg):
    """sc_hypothesize_begin_device / _end_device (include/saccot.h): every rank samples its share of the pruning
    certificate, the histograms are summed (the 1 KiB all-reduce, done on the host here), and the rest runs as usual.
    The summed histogram must equal the one a single rank builds, and winner, (R,t) and mask the unsharded run's."""
    import torch
    cfg, scene = pkg.synth.make_config_scene("C1")
    kw = cfg.params()
    base = reg.register(scene.src, scene.tgt, **kw)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    d_key = torch.zeros(2, dtype=torch.int64, device=dev)
    d_hist = torch.zeros(pkg.SC_HIST_WORDS, dtype=torch.int32, device=dev)
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(cfg.n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    full = None
    for world in (1, 2, 5):
        parts = []
        for rank in range(world):
            p = pkg.make_params(shard_rank=rank, shard_world=world, shard_block=256, **kw)
            reg.hypothesize_begin_device(d_src.data_ptr(), d_tgt.data_ptr(), cfg.n, p, d_hist.data_ptr())
            torch.cuda.synchronize()
            parts.append(d_hist.cpu().numpy().view(np.uint32).astype(np.uint64))
        total = sum(parts)
        assert total.sum() > 0 and all(q.sum() > 0 for q in parts)     # every rank really sampled something
        if full is None:
            full = total                                                # world 1: the whole sample
        assert np.array_equal(total, full)                              # shares partition the sample exactly
        summed = torch.from_numpy((total & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)).to(dev)
        keys, scored = [], 0
        for rank in range(world):
            p = pkg.make_params(shard_rank=rank, shard_world=world, shard_block=256, **kw)
            reg.hypothesize_begin_device(d_src.data_ptr(), d_tgt.data_ptr(), cfg.n, p, d_hist.data_ptr())
            d_hist.copy_(summed)                                        # what shard.allreduce_hist leaves on every rank
            torch.cuda.synchronize()
            st = reg.hypothesize_end_device(d_hist.data_ptr(), d_key.data_ptr())
            torch.cuda.synchronize()
            keys.append(tuple(int(x) for x in d_key.cpu())); scored += st["tri_scored"]
        assert scored == base["stats"]["tri_kept"]
        k0, k1 = pkg.shard.reduce_pairs(keys)
        d_key.copy_(torch.tensor([k0, k1], dtype=torch.int64)); torch.cuda.synchronize()
        rc, st = reg.finalize_device(d_key.data_ptr(), d_Rt.data_ptr(), d_mask.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and st["best_rank"] == base["stats"]["best_rank"] and st["best_count"] == base["stats"]["best_count"]
        assert np.array_equal(d_mask.cpu().numpy(), base["mask"])
        assert d_Rt.cpu().numpy().tobytes() == np.concatenate([base["R"].ravel(), base["t"]]).tobytes()
    with pytest.raises(pkg.SacCotError):                                # end without begin
        reg.hypothesize_end_device(d_hist.data_ptr(), d_key.data_ptr())


@pytest.mark.parametrize("name,extra", [("C0", {}), ("C1", {"rank_mode": 1}), ("C1", {"flags": 4})])
def test_split_phase1_without_pruning_and_gathered_finalize(pkg, reg, name, extra):
    """begin/end where the certificate does not run (a graph below 4096 edges, degree ranking, SC_FLAG_NO_PRUNE): the
    histogram stays zero and is ignored; the gathered finalize (two ranks' pairs, one of them 'no hypothesis') must
    give the unsharded result, and an all-zero gather must report SC_ENOHYP with identity / zero mask."""
    import torch
    cfg, scene = pkg.synth.make_config_scene(name)
    kw = dict(cfg.params(), **{k: v for k, v in extra.items() if k != "flags"})
    flags = extra.get("flags", 0)
    base = reg.register(scene.src, scene.tgt, flags=flags, **kw)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    d_key = torch.zeros(2, dtype=torch.int64, device=dev)
    d_hist = torch.ones(pkg.SC_HIST_WORDS, dtype=torch.int32, device=dev)        # begin must zero it
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(cfg.n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = pkg.make_params(flags=flags, **kw)
    reg.hypothesize_begin_device(d_src.data_ptr(), d_tgt.data_ptr(), cfg.n, p, d_hist.data_ptr())
    torch.cuda.synchronize()
    pruned = kw.get("rank_mode", 0) == 0 and not (flags & 4) and base["stats"]["edges"] >= 4096
    assert (int(d_hist.abs().sum()) > 0) == pruned
    reg.hypothesize_end_device(d_hist.data_ptr(), d_key.data_ptr())
    torch.cuda.synchronize()
    mine = [int(x) for x in d_key.cpu()]
    d_all = torch.tensor([0, 0] + mine, dtype=torch.int64).to(dev); torch.cuda.synchronize()   # rank 0: nothing, rank 1: ours
    rc, st = reg.finalize_gathered_device(d_all.data_ptr(), 2, d_Rt.data_ptr(), d_mask.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and (st["best_rank"], st["best_count"]) == (base["stats"]["best_rank"], base["stats"]["best_count"])
    assert np.array_equal(d_mask.cpu().numpy(), base["mask"])
    assert d_Rt.cpu().numpy().tobytes() == np.concatenate([base["R"].ravel(), base["t"]]).tobytes()
    d_all.zero_(); torch.cuda.synchronize()
    rc, st = reg.finalize_gathered_device(d_all.data_ptr(), 2, d_Rt.data_ptr(), d_mask.data_ptr())
    torch.cuda.synchronize()
    assert rc == pkg.SC_ENOHYP and int(d_mask.sum()) == 0
    assert np.array_equal(d_Rt.cpu().numpy(), np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32))


@pytest.mark.parametrize("n_pairs", [9, 40, 300, 4096])
def test_finalize_reduces_many_gathered_pairs_like_few(pkg, reg, n_pairs):
    """r05: more than eight key pairs are reduced by the whole workgroup (a thread takes every 256th pair) instead of one scalar loop —
    the form this context's own arg-max launch now feeds (one pair per workgroup).  The lexicographic maximum must come out wherever
    the winning pair sits, with ties on the first word decided by the second, and an out-of-range pair must still be refused."""
    import torch
    cfg, scene = pkg.synth.make_config_scene("C0")
    kw = cfg.params()
    base = reg.register(scene.src, scene.tgt, **kw)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    d_key = torch.zeros(2, dtype=torch.int64, device=dev)
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(cfg.n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    reg.hypothesize_device(d_src.data_ptr(), d_tgt.data_ptr(), cfg.n, pkg.make_params(**kw), d_key.data_ptr())
    torch.cuda.synchronize()
    good = [int(x) for x in d_key.cpu()]
    rng = np.random.default_rng(n_pairs)
    for where in (0, n_pairs // 2, n_pairs - 1):
        pairs = np.zeros((n_pairs, 2), dtype=np.int64)
        for k in range(n_pairs):                     # losers: the same first word with a smaller second, smaller first words, empty pairs
            kind = rng.integers(0, 3)
            if kind == 0:
                pairs[k] = (good[0], max(good[1] - int(rng.integers(1, 1000)), 0))
            elif kind == 1:
                pairs[k] = (max(good[0] - (int(rng.integers(1, 50)) << 32), 1), good[1] + int(rng.integers(0, 1000)))
        pairs[where] = good
        d_all = torch.from_numpy(pairs.reshape(-1)).to(dev); torch.cuda.synchronize()
        rc, st = reg.finalize_gathered_device(d_all.data_ptr(), n_pairs, d_Rt.data_ptr(), d_mask.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and (st["best_rank"], st["best_count"]) == (base["stats"]["best_rank"], base["stats"]["best_count"]), (n_pairs, where)
        assert np.array_equal(d_mask.cpu().numpy(), base["mask"])
        assert d_Rt.cpu().numpy().tobytes() == np.concatenate([base["R"].ravel(), base["t"]]).tobytes()
    pairs[n_pairs // 3] = (good[0] + (1 << 40), 0xFFFFFFFF - (base["stats"]["tri_kept"] + 7))   # wins the reduction, points outside
    d_all = torch.from_numpy(pairs.reshape(-1)).to(dev); torch.cuda.synchronize()
    with pytest.raises(pkg.SacCotError) as e:
        reg.finalize_gathered_device(d_all.data_ptr(), n_pairs, d_Rt.data_ptr(), d_mask.data_ptr())
    assert e.value.status == pkg.SC_EINVAL


def test_finalize_rejects_a_pair_outside_the_selection(pkg, reg):
    """The key pairs of phase 2 come from the caller (an all-gather).  A pair whose position lies outside the selected
    list — a stale or uninitialised buffer, ranks that disagree on T — must not be used as an index on the device: the
    call returns SC_EINVAL with identity / zero mask, and the context stays usable."""
    import torch
    cfg, scene = pkg.synth.make_config_scene("C0")
    kw = cfg.params()
    base = reg.register(scene.src, scene.tgt, **kw)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    d_key = torch.zeros(2, dtype=torch.int64, device=dev)
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.ones(cfg.n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = pkg.make_params(**kw)
    reg.hypothesize_device(d_src.data_ptr(), d_tgt.data_ptr(), cfg.n, p, d_key.data_ptr())
    torch.cuda.synchronize()
    good = [int(x) for x in d_key.cpu()]
    T_eff = base["stats"]["tri_kept"]
    for pos in (T_eff, T_eff + 12345, 0xFFFFFFFF):                      # first position outside, far outside, maximal
        bad = [good[0] + (1 << 40), 0xFFFFFFFF - pos]                   # more inliers than anyone: it wins the reduction
        d_all = torch.tensor(good + bad, dtype=torch.int64).to(dev); torch.cuda.synchronize()
        with pytest.raises(pkg.SacCotError) as e:
            reg.finalize_gathered_device(d_all.data_ptr(), 2, d_Rt.data_ptr(), d_mask.data_ptr())
        assert e.value.status == pkg.SC_EINVAL
        torch.cuda.synchronize()
        assert int(d_mask.sum()) == 0
        assert np.array_equal(d_Rt.cpu().numpy(), np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32))
    d_all = torch.tensor(good + [0, 0], dtype=torch.int64).to(dev); torch.cuda.synchronize()
    rc, st = reg.finalize_gathered_device(d_all.data_ptr(), 2, d_Rt.data_ptr(), d_mask.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(d_mask.cpu().numpy(), base["mask"])


def test_caller_stream_orders_torch_work_with_the_kernels(pkg):
    """sc_set_stream: on torch's current stream (the default stream, which torch reports as 0 and api.py maps to
    SC_STREAM_DEFAULT, and a side stream) torch's own work on that stream is ordered with the library's kernels: the
    key pair read back by torch right after hypothesize_device — no explicit synchronisation — is the final one."""
    import torch
    cfg, scene = pkg.synth.make_config_scene("C1")
    dev = torch.device("cuda:0")
    r = pkg.Registrar(0)
    try:
        base = r.register(scene.src, scene.tgt, **cfg.params())
        d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
        p = pkg.make_params(**cfg.params())
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        for stream in (torch.cuda.current_stream(dev), side):
            with torch.cuda.stream(stream):
                r.set_stream(stream.cuda_stream)
                d_key = torch.zeros(2, dtype=torch.int64, device=dev)
                d_Rt = torch.zeros(12, dtype=torch.float32, device=dev)
                d_mask = torch.zeros(cfg.n, dtype=torch.uint8, device=dev)
                for _ in range(3):
                    d_key.zero_()
                    r.hypothesize_device(d_src.data_ptr(), d_tgt.data_ptr(), cfg.n, p, d_key.data_ptr())
                    k = d_key.clone()                          # torch work on the same stream: ordered after the arg-max
                    rc, st = r.finalize_device(d_key.data_ptr(), d_Rt.data_ptr(), d_mask.data_ptr())
                    m = d_mask.clone()
                    k0 = int(k.cpu()[0])
                    assert (k0 >> 32) == base["stats"]["best_count"] and rc == 0
                    assert np.array_equal(m.cpu().numpy(), base["mask"])
        r.set_stream(None)
    finally:
        r.close()


def test_errors(pkg, reg):
    cfg, scene = pkg.synth.make_config_scene("C0")
    with pytest.raises(pkg.SacCotError) as e:
        reg.register(scene.src[:2], scene.tgt[:2], **cfg.params())          # n < 3
    assert e.value.status == pkg.SC_EINVAL
    bad = scene.src.copy(); bad[17, 1] = np.nan
    with pytest.raises(pkg.SacCotError) as e:
        reg.register(bad, scene.tgt, **cfg.params())                          # non-finite input
    assert e.value.status == pkg.SC_EINVAL
    with pytest.raises(pkg.SacCotError) as e:
        reg.register(scene.src, scene.tgt, **dict(cfg.params(), t_cmp=1.5))   # bad parameter
    assert e.value.status == pkg.SC_EINVAL
    out = reg.register(scene.src, scene.tgt, **cfg.params())                   # context still usable
    assert out["status"] == 0


def test_rigid_motion_invariance_of_graph(pkg, reg):
    """Property: moving the target cloud rigidly leaves the edge set unchanged away from the thresholds."""
    cfg, scene = pkg.synth.make_config_scene("C0")
    p = pkg.make_params(**cfg.params())
    _, bits, _ = reg.compat(scene.src, scene.tgt, p, want_S=False)
    th = 0.7
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    tgt2 = (scene.tgt.astype(np.float64) @ Rz.T + np.array([0.3, -0.2, 0.1])).astype(np.float32)
    _, bits2, _ = reg.compat(scene.src, tgt2, p, want_S=False)
    diff = sum(bin(int(x)).count("1") for x in (bits ^ bits2).ravel())
    total = sum(bin(int(x)).count("1") for x in bits.ravel())
    assert diff <= 0.002 * total + 4   # only threshold-edge pairs may flip under fp32 re-rounding


# ---------------------------------------------------------------------------------------------------------
# the matrix-pipe variant of C2 and the big configs
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["256", "96"])
def test_score_mfma_variant_bit_exact(pkg, O, split):
    """the f32-MFMA scoring body (v_mfma_f32_16x16x4_f32, C = -q) must count exactly like the VALU
    body.  sc_debug.score_split sends that share (of 256) of the hypotheses to MFMA workgroups."""
    reg = pkg.Registrar(0)
    reg.set_debug(score_split=int(split))
    n, T = 1300, 5000
    sc = _scene(pkg, n, seed=91)
    rng = np.random.default_rng(91)
    inl = np.nonzero(sc.inlier)[0]
    tri = np.sort(np.stack([rng.choice(inl if h % 2 else n, 3, replace=False) for h in range(T)]), axis=1).astype(np.uint32)
    Rt0 = O.kabsch3(sc.src, sc.tgt, tri)
    Rt0[11, 2] = np.inf; Rt0[4000, 9] = np.nan
    kw = _params(pkg, 0.05, T)
    cnt, key = reg.score(sc.src, sc.tgt, pkg.make_params(**kw), Rt0)
    cnt0 = O.score(sc.src, sc.tgt, Rt0, kw["tau"])
    assert cnt0.max() > 50 and cnt0[11] == 0 and cnt0[4000] == 0
    assert np.array_equal(cnt, cnt0) and key == O.best_key(cnt0)
    cfg, scene = pkg.synth.make_config_scene("C1")
    _check_register(pkg, O, reg, scene, cfg.params())
    reg.close()


def test_register_C4_half_a_million_hypotheses(pkg, O, reg):
    """BASELINE.json configs[4]: N = 5000 with 90 % outliers, 500k ranked triangles (one GPU scores them all here)."""
    cfg, scene = pkg.synth.make_config_scene("C4")
    got, ref = _check_register(pkg, O, reg, scene, cfg.params())
    assert got["stats"]["tri_kept"] == 500_000 and got["stats"]["tri_scored"] == 500_000
    assert pkg.synth.rotation_error_deg(got["R"], scene.R_gt) < 1.0


def test_register_C3_twenty_thousand_correspondences(pkg, O, reg):
    """BASELINE.json configs[3]: N = 20000 (1.6 GB weight matrix, ~4e8 triangles in the graph), 200k hypotheses."""
    cfg, scene = pkg.synth.make_config_scene("C3")
    got, ref = _check_register(pkg, O, reg, scene, cfg.params(), threads=64)
    assert got["stats"]["tri_kept"] == 200_000
    assert pkg.synth.rotation_error_deg(got["R"], scene.R_gt) < 1.0
    m = got["mask"].astype(bool)
    assert (m & scene.inlier).sum() >= 0.95 * scene.inlier.sum()


def test_event_buffer_overflow_falls_back_to_row_walk(pkg, O):
    """Stage B's event list has a fixed capacity per call; when a region overflows, the call must fall back to the
    row-walking key kernel (and grow the buffer for next time) with identical results.  sc_debug.event_cap forces a
    buffer far too small for C1/C2; sc_debug.no_events disables the event path altogether."""
    cfg, scene = pkg.synth.make_config_scene("C2")
    ref = O.register(scene.src, scene.tgt, threads=8, **cfg.params())
    for knobs in (dict(event_cap=4096), dict(no_events=1)):
        r = pkg.Registrar(0)   # fresh context: default capacities
        try:
            r.set_debug(**knobs)
            for _ in range(2):  # second call runs with the capacity the first one asked for (knob still forces it small)
                got = r.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_EXACT_TOTAL, **cfg.params())
                assert got["status"] == 0 and got["stats"]["best_rank"] == ref["best_rank"]
                assert np.array_equal(got["mask"], ref["mask"]) and nan_equal_bits(got["R"], ref["R"]) and nan_equal_bits(got["t"], ref["t"])
                assert got["stats"]["tri_total"] == ref["tri_total"]
        finally:
            r.close()


@pytest.mark.parametrize("name", ["C0", "C1", "C2"])
def test_refine_matches_oracle_and_improves(pkg, O, reg, name):
    """SURVEY §8f-2 (SC_FLAG_REFINE): the fp64 least-squares refit over the winner's inliers must equal the oracle's
    (same chunked summation order) bit for bit after rounding to fp32, leave the mask alone, and not be worse than the
    3-point hypothesis against the synthetic ground truth."""
    cfg, scene = pkg.synth.make_config_scene(name)
    base = reg.register(scene.src, scene.tgt, **cfg.params())
    got = reg.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_REFINE, **cfg.params())
    assert np.array_equal(got["mask"], base["mask"]) and got["stats"]["best_rank"] == base["stats"]["best_rank"]
    done, Rt0 = O.refine(scene.src, scene.tgt, base["mask"], np.concatenate([base["R"].ravel(), base["t"]]))
    assert done
    assert np.concatenate([got["R"].ravel(), got["t"]]).astype(np.float32).tobytes() == Rt0.tobytes()
    e0 = pkg.synth.rotation_error_deg(base["R"], scene.R_gt); e1 = pkg.synth.rotation_error_deg(got["R"], scene.R_gt)
    assert e1 <= e0 + 1e-3 and e1 < 0.5
    assert np.linalg.norm(got["t"] - scene.t_gt) <= np.linalg.norm(base["t"] - scene.t_gt) + 1e-4


# ---------------------------------------------------------------------------------------------------------
# stages A and B sharded: the phase API, every "rank" a context of its own on this one GPU
# ---------------------------------------------------------------------------------------------------------
def _run_sharded_ab(pkg, n, kw, d_src, d_tgt, world, flags=0, regs=None, block=256, level=0, levels_out=None):
    """(see _run_sharded_ab_once)  SC_ERETRY — a candidate blob was too small — raises the level and runs again, as a
    caller must; levels_out (a list) receives the level the call ended with."""
    for _ in range(24):
        out = _run_sharded_ab_once(pkg, n, dict(kw, shard_cand_level=level), d_src, d_tgt, world, flags, regs, block)
        if out[0] != pkg.SC_ERETRY:
            if levels_out is not None:
                levels_out.append(level)
            return out
        level += 1
    raise AssertionError("SC_ERETRY did not end")


def _run_sharded_ab_once(pkg, n, kw, d_src, d_tgt, world, flags=0, regs=None, block=256):
    """The whole sharded call for `world` ranks on one GPU.  The ranks share the exchange buffers, which is exactly what
    the collectives deliver: the in-place all-gather of the bit rows and of the candidate blobs are no-ops here, the
    histogram all-reduce is a host-side sum.  Returns (rc, stats, Rt, mask, per-rank enumerated)."""
    import torch
    dev = torch.device("cuda:0")
    own = regs is None
    regs = regs or [pkg.Registrar(0) for _ in range(world)]
    try:
        ps = [pkg.make_params(shard_rank=r, shard_world=world, shard_block=block, flags=flags, **kw) for r in range(world)]
        plan = pkg.shard_plan(ps[0], n)
        d_bits = torch.zeros(plan.bits_bytes_total // 8, dtype=torch.int64, device=dev)
        d_hists = [torch.zeros(pkg.SC_HIST_WORDS, dtype=torch.int32, device=dev) for _ in range(world)]
        d_cand = torch.zeros(world * plan.cand_bytes_per_rank // 8, dtype=torch.int64, device=dev)
        d_keys = torch.zeros(2 * world, dtype=torch.int64, device=dev)
        d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for r in range(world):
            regs[r].shard_compat_device(d_src.data_ptr(), d_tgt.data_ptr(), n, ps[r], d_bits.data_ptr())
        torch.cuda.synchronize()                                   # (all-gather of the bit rows: shared buffer)
        for r in range(world):
            regs[r].shard_edges_device(d_hists[r].data_ptr())
        torch.cuda.synchronize()
        if flags & pkg.SC_FLAG_EST_BOUND:                          # every rank took the whole sample: NO all-reduce, identical histograms
            h0 = d_hists[0].cpu().numpy()
            assert all(np.array_equal(h.cpu().numpy(), h0) for h in d_hists[1:])
        else:
            total = sum(h.cpu().numpy().view(np.uint32).astype(np.uint64) for h in d_hists)
            summed = torch.from_numpy((total & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)).to(dev)
            for r in range(world):                                 # (all-reduce SUM of the sample histograms)
                d_hists[r].copy_(summed)
        torch.cuda.synchronize()
        for r in range(world):
            regs[r].shard_select_device(d_hists[r].data_ptr(), d_cand.data_ptr() + r * plan.cand_bytes_per_rank)
        torch.cuda.synchronize()                                   # (all-gather of the candidate blobs: shared buffer)
        hdr = d_cand.cpu().numpy().view(np.uint64).reshape(world, -1)[:, :2]
        scored = 0
        for r in range(world):
            st = regs[r].shard_score_device(d_cand.data_ptr(), d_keys.data_ptr() + 16 * r)
            scored += st["tri_scored"]
        torch.cuda.synchronize()                                   # (all-gather of the key pairs: shared buffer)
        out = []
        for r in range(world):
            rc, st = regs[r].finalize_gathered_device(d_keys.data_ptr(), world, d_Rt.data_ptr(), d_mask.data_ptr())
            torch.cuda.synchronize()
            out.append((rc, st, d_Rt.cpu().numpy().copy(), d_mask.cpu().numpy().copy()))
        for o in out[1:]:                                          # every rank ends with the same answer
            assert o[0] == out[0][0]
            if o[0] not in (pkg.SC_ERETRY, pkg.SC_EBOUND):
                assert o[2].tobytes() == out[0][2].tobytes() and np.array_equal(o[3], out[0][3])
                assert o[1]["best_rank"] == out[0][1]["best_rank"]
        rc, st, Rt, mask = out[0]
        if rc not in (pkg.SC_ERETRY, pkg.SC_EBOUND):
            assert scored == st["tri_kept"]
        return rc, st, Rt, mask, hdr
    finally:
        if own:
            for g in regs:
                g.close()


@pytest.mark.parametrize("name,worlds", [("C0", (1, 2, 5)), ("C1", (1, 2, 3, 8)), ("C2", (2, 8))])
def test_sharded_A_and_B_equal_unsharded(pkg, O, reg, name, worlds):
    """stage A by row blocks, stage B by contiguous row ranges, candidates merged with the same total
    order.  For every world size the winner, its rank index, (R,t) and the mask must equal the unsharded run's (and the
    CPU restatement's) bit for bit, and the ranks' row ranges must partition the enumeration."""
    import torch
    cfg, scene = pkg.synth.make_config_scene(name)
    kw = cfg.params()
    certified = pkg.Registrar(0); certified.set_debug(no_estimate=1)   # the phase API certifies its pruning bound: so must the base
    base = certified.register(scene.src, scene.tgt, **kw)
    certified.close()
    ref = O.register(scene.src, scene.tgt, threads=8, **kw)
    assert base["stats"]["best_rank"] == ref["best_rank"]
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    for world in worlds:
        rc, st, Rt, mask, hdr = _run_sharded_ab(pkg, cfg.n, kw, d_src, d_tgt, world)
        assert rc == 0, world
        assert (st["best_rank"], st["best_count"], st["tri_kept"]) == (ref["best_rank"], ref["best_count"], ref["t_eff"]), world
        assert st["edges"] == ref["edges"] and np.array_equal(mask, ref["mask"]), world
        assert Rt.tobytes() == np.concatenate([ref["R"].ravel(), ref["t"]]).astype(np.float32).tobytes(), world
        assert int(hdr[:, 0].sum()) == st["tri_total"] == base["stats"]["tri_total"], world   # the ranges partition the enumeration
        if world > 1 and name != "C0":
            share = hdr[:, 0].astype(np.float64) / hdr[:, 0].sum()
            assert share.max() < 2.5 / world, (world, share)        # equally heavy row ranges, roughly


@pytest.mark.parametrize("name,worlds", [("C1", (2, 3, 8)), ("C2", (2, 8)), ("C4", (8,))])
def test_sharded_with_an_estimated_bound_equals_unsharded(pkg, O, name, worlds):
    """SC_FLAG_EST_BOUND: every rank takes the whole estimating sample (identical histograms, NO all-reduce: three collectives
    per call), prunes by the estimated bound, and the merge verifies it.  Same winner, (R,t), mask and selection as the
    oracle's; fewer triangles enumerated than with the certified bound.  Then the failure path: an estimate aimed at rank
    T / 100 (sc_debug.est_margin_pct on every rank) must come back as SC_EBOUND from EVERY rank, and the same call without the
    flag succeeds."""
    import torch
    cfg, scene = pkg.synth.make_config_scene(name)
    kw = cfg.params()
    ref = O.register(scene.src, scene.tgt, threads=8, **kw)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    for world in worlds:
        rc, st, Rt, mask, hdr = _run_sharded_ab(pkg, cfg.n, kw, d_src, d_tgt, world, flags=pkg.SC_FLAG_EST_BOUND)
        assert rc == 0, world
        assert (st["best_rank"], st["best_count"], st["tri_kept"]) == (ref["best_rank"], ref["best_count"], ref["t_eff"]), world
        assert np.array_equal(mask, ref["mask"]) and Rt.tobytes() == np.concatenate([ref["R"].ravel(), ref["t"]]).astype(np.float32).tobytes()
        rc2, st2, _, _, hdr2 = _run_sharded_ab(pkg, cfg.n, kw, d_src, d_tgt, world)
        assert rc2 == 0 and int(hdr[:, 0].sum()) == st["tri_total"]
        print(name, "world", world, "enumerated: estimated bound", st["tri_total"], "certified", st2["tri_total"])
    world = worlds[0]
    regs = [pkg.Registrar(0) for _ in range(world)]
    try:
        for g in regs:
            g.set_debug(est_margin_pct=1)
        out = _run_sharded_ab_once(pkg, cfg.n, dict(kw, shard_cand_level=0), d_src, d_tgt, world, flags=pkg.SC_FLAG_EST_BOUND, regs=regs)
        assert out[0] == pkg.SC_EBOUND
        out = _run_sharded_ab_once(pkg, cfg.n, dict(kw, shard_cand_level=0), d_src, d_tgt, world, regs=regs)
        assert out[0] == 0 and out[1]["best_rank"] == ref["best_rank"] and np.array_equal(out[3], ref["mask"])
    finally:
        for g in regs:
            g.close()


@pytest.mark.parametrize("knobs", [dict(), dict(sample_mode=1), dict(no_estimate=1), dict(no_events=1)])
def test_sharded_with_the_flag_where_the_plan_is_no_estimate_still_gives_every_rank_the_same_histogram(pkg, O, knobs):
    """SC_FLAG_EST_BOUND makes the callers skip the histogram all-reduce.  Where the plan is NOT an estimate —
    the select window unknown (t_cmp = 0.6 < 0.668), or sc_debug asks for a certifying form — every rank used to take only ITS
    share of the sample, derived its own bound and cut the strong list its own way.  Every rank now takes the whole certifying
    sample: identical histograms (asserted inside the helper), results bit-identical to the single-GPU call and the oracle."""
    import torch
    cfg, scene = pkg.synth.make_config_scene("C1")
    kw = dict(cfg.params(), t_cmp=0.9 if knobs else 0.6)
    ref = O.register(scene.src, scene.tgt, threads=8, **kw)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    for world in (2, 4):
        regs = [pkg.Registrar(0) for _ in range(world)]
        try:
            for g in regs:
                if knobs:
                    g.set_debug(**knobs)
            rc, st, Rt, mask, _ = _run_sharded_ab_once(pkg, cfg.n, dict(kw, shard_cand_level=0), d_src, d_tgt, world, flags=pkg.SC_FLAG_EST_BOUND, regs=regs)
        finally:
            for g in regs:
                g.close()
        assert rc == ref["rc"] == 0, (world, rc)
        assert (st["best_rank"], st["best_count"], st["tri_kept"]) == (ref["best_rank"], ref["best_count"], ref["t_eff"]), world
        assert np.array_equal(mask, ref["mask"]) and Rt.tobytes() == np.concatenate([ref["R"].ravel(), ref["t"]]).astype(np.float32).tobytes()


@pytest.mark.parametrize("extra", [dict(rank_mode=1), dict(flags=4), dict(flags=32), dict(t_cmp=0.5), dict(max_triangles=10_000_000)])
def test_sharded_A_and_B_other_modes(pkg, O, extra):
    """The sharded phases where the certificate does not run (degree ranking, SC_FLAG_NO_PRUNE), without the dense
    matrix, with the key window taken from the data (t_cmp < 2/3) and with T larger than the number of triangles."""
    import torch
    cfg, scene = pkg.synth.make_config_scene("C1" if "max_triangles" not in extra else "C0")
    kw = dict(cfg.params(), **{k: v for k, v in extra.items() if k != "flags"})
    flags = extra.get("flags", 0)
    ref = O.register(scene.src, scene.tgt, threads=8, **kw)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    for world in (2, 3):
        rc, st, Rt, mask, _ = _run_sharded_ab(pkg, cfg.n, kw, d_src, d_tgt, world, flags=flags)
        assert rc == ref["rc"] == 0
        assert (st["best_rank"], st["best_count"], st["tri_kept"]) == (ref["best_rank"], ref["best_count"], ref["t_eff"])
        assert np.array_equal(mask, ref["mask"])
        assert Rt.tobytes() == np.concatenate([ref["R"].ravel(), ref["t"]]).astype(np.float32).tobytes()


def test_sharded_A_and_B_massive_ties_and_no_triangles(pkg, O):
    """Ties decide almost the whole selection on a noise-free all-inlier scene (the concatenation order of the blobs
    must then BE the (i,j,k) order), and a scene without any edge must end in SC_ENOHYP on every rank."""
    import torch
    dev = torch.device("cuda:0")
    sc = pkg.synth.make_scene(150, 1.0, 1.0, 1e-7, 21)
    kw = _params(pkg, 0.05, 3000)
    ref = O.register(sc.src, sc.tgt, threads=4, **kw)
    d_src = torch.from_numpy(sc.src).to(dev); d_tgt = torch.from_numpy(sc.tgt).to(dev)
    for world in (2, 4):
        rc, st, Rt, mask, _ = _run_sharded_ab(pkg, 150, kw, d_src, d_tgt, world, block=64)
        assert rc == 0 and (st["best_rank"], st["best_count"], st["tri_kept"]) == (ref["best_rank"], ref["best_count"], ref["t_eff"])
        assert np.array_equal(mask, ref["mask"]) and Rt.tobytes() == np.concatenate([ref["R"].ravel(), ref["t"]]).astype(np.float32).tobytes()
    rng = np.random.default_rng(5)
    src = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    tgt = (src * 37.0).astype(np.float32)
    d_src = torch.from_numpy(src).to(dev); d_tgt = torch.from_numpy(tgt).to(dev)
    rc, st, Rt, mask, _ = _run_sharded_ab(pkg, 40, _params(pkg, 0.001, 100), d_src, d_tgt, 2)
    assert rc == pkg.SC_ENOHYP and not mask.any() and st["edges"] == 0


# ---------------------------------------------------------------------------------------------------------
# native multi-device entry (sc_create_multi / sc_register_multi): one device, and the loopback transport
# ---------------------------------------------------------------------------------------------------------
def test_multi_one_device_is_sc_register(pkg, reg):
    """n_dev == 1 makes no RCCL call and is exactly sc_register."""
    cfg, scene = pkg.synth.make_config_scene("C1")
    base = reg.register(scene.src, scene.tgt, **cfg.params())
    m = pkg.MultiRegistrar((0,))
    try:
        got = m.register(scene.src, scene.tgt, **cfg.params())
    finally:
        m.close()
    assert got["status"] == 0 and np.array_equal(got["mask"], base["mask"])
    assert got["R"].tobytes() == base["R"].tobytes() and got["t"].tobytes() == base["t"].tobytes()
    assert got["stats"]["best_rank"] == base["stats"]["best_rank"]
    with pytest.raises(pkg.SacCotError) as e:                     # one rank per device
        pkg.MultiRegistrar((0, 0))
    assert e.value.status == pkg.SC_EINVAL


@pytest.mark.parametrize("ranks", [1, 2, 3, 5])
def test_multi_loopback_equals_sc_register(pkg, O, reg, ranks):
    """sc_create_multi_loopback: `ranks` ranks on this one GPU, worker thread each, device copies in place of the RCCL
    collectives — buffers, phase order, error agreement and outputs of sc_register_multi, bit for bit against
    sc_register and the CPU restatement (ranks == 1: the same machinery over a real single-rank RCCL communicator, so
    librccl is opened and ncclCommInitAll / ncclAllGather / ncclAllReduce really execute); then an input error (every rank must report it, nobody may hang), a scene
    without hypotheses, and the handle reused for another size."""
    m = pkg.MultiRegistrar((0,), loopback_ranks=ranks)
    try:
        # both forms of the multi-device call: stages A and B replicated with the estimated bound (the default below 8192
        # correspondences, r04b: one key-pair exchange) and all three stages sharded (SC_FLAG_SHARD_AB: three or four collectives)
        for name, fl in (("C1", 0), ("C1", pkg.SC_FLAG_SHARD_AB), ("C0", pkg.SC_FLAG_SHARD_AB), ("C0", 0)):
            cfg, scene = pkg.synth.make_config_scene(name)
            ref = O.register(scene.src, scene.tgt, threads=8, **cfg.params())
            got = m.register(scene.src, scene.tgt, flags=fl, **cfg.params())
            assert got["status"] == ref["rc"] == 0
            st = got["stats"]
            assert (st["edges"], st["tri_kept"], st["best_rank"], st["best_count"]) == (ref["edges"], ref["t_eff"], ref["best_rank"], ref["best_count"])
            assert st["tri_scored"] == ref["t_eff"]                                   # summed over the ranks
            assert np.array_equal(got["mask"], ref["mask"]) and nan_equal_bits(got["R"], ref["R"]) and nan_equal_bits(got["t"], ref["t"])
        bad = scene.src.copy(); bad[3, 0] = np.inf
        with pytest.raises(pkg.SacCotError) as e:
            m.register(bad, scene.tgt, **cfg.params())
        assert e.value.status == pkg.SC_EINVAL
        rng = np.random.default_rng(5)
        src = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
        out = m.register(src, (src * 37.0).astype(np.float32), **_params(pkg, 0.001, 100))
        assert out["status"] == pkg.SC_ENOHYP and not out["mask"].any()
        got = m.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_REFINE | pkg.SC_FLAG_NO_DENSE_S, **cfg.params())
        base = reg.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_REFINE, **cfg.params())
        assert got["R"].tobytes() == base["R"].tobytes() and np.array_equal(got["mask"], base["mask"])
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------
# SURVEY §8f-2 `score_mode`: truncated squared / absolute residual instead of the inlier count
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_score_modes_bit_exact(pkg, O, reg, mode):
    """Every hypothesis' truncated score (an exact integer sum), the winner key, and the whole path — unsharded, sharded
    A + B and through the multi-device loopback — against the CPU restatement."""
    import torch
    n, T = 1100, 3000
    sc = _scene(pkg, n, seed=n)
    rng = np.random.default_rng(n)
    inl = np.nonzero(sc.inlier)[0]
    tri = np.sort(np.stack([rng.choice(inl if h % 2 else n, 3, replace=False) for h in range(T)]), axis=1).astype(np.uint32)
    Rt0 = O.kabsch3(sc.src, sc.tgt, tri)
    Rt0[5, 1] = np.nan
    kw = _params(pkg, 0.05, T)
    cnt, key = reg.score(sc.src, sc.tgt, pkg.make_params(score_mode=mode, **kw), Rt0)
    cnt0 = O.score(sc.src, sc.tgt, Rt0, kw["tau"], score_mode=mode)
    assert cnt0.max() > 50_000 and cnt0[5] == 0
    assert np.array_equal(cnt, cnt0) and key == O.best_key(cnt0)
    for name in ("C0", "C1", "C2"):
        cfg, scene = pkg.synth.make_config_scene(name)
        ref = O.register(scene.src, scene.tgt, threads=8, score_mode=mode, **cfg.params())
        got = reg.register(scene.src, scene.tgt, score_mode=mode, **cfg.params())
        assert got["status"] == ref["rc"] == 0
        assert (got["stats"]["best_rank"], got["stats"]["best_count"]) == (ref["best_rank"], ref["best_count"])
        assert np.array_equal(got["mask"], ref["mask"]) and nan_equal_bits(got["R"], ref["R"]) and nan_equal_bits(got["t"], ref["t"])
        assert got["stats"]["best_count"] <= 1024 * int(ref["mask"].sum())
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    rc, st, Rt, mask, _ = _run_sharded_ab(pkg, cfg.n, dict(cfg.params(), score_mode=mode), d_src, d_tgt, 3)
    assert rc == 0 and (st["best_rank"], st["best_count"]) == (ref["best_rank"], ref["best_count"]) and np.array_equal(mask, ref["mask"])
    m = pkg.MultiRegistrar((0,), loopback_ranks=2)
    try:
        out = m.register(scene.src, scene.tgt, score_mode=mode, **cfg.params())
    finally:
        m.close()
    assert out["stats"]["best_rank"] == ref["best_rank"] and np.array_equal(out["mask"], ref["mask"])


def test_known_answer_bars_per_mode(pkg, reg):
    """SURVEY §8c known-answer bars on synthetic ground truth, stated per mode: a raw 3-point hypothesis is coarse
    (rotation < 3 deg, mask covers >= 90 % of the true inliers); with SC_FLAG_REFINE (the least-squares refit over the
    winner's inliers) the survey's bars hold: rotation < 0.5 deg, translation < tau, mask >= 95 % of the true inliers."""
    for name in ("C0", "C1", "C2"):
        cfg, scene = pkg.synth.make_config_scene(name)
        raw = reg.register(scene.src, scene.tgt, **cfg.params())
        ref = reg.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_REFINE, **cfg.params())
        assert pkg.synth.rotation_error_deg(raw["R"], scene.R_gt) < 3.0
        assert (raw["mask"].astype(bool) & scene.inlier).sum() >= 0.90 * scene.inlier.sum()
        assert pkg.synth.rotation_error_deg(ref["R"], scene.R_gt) < 0.5
        assert np.linalg.norm(ref["t"] - scene.t_gt) < cfg.tau
        # the refit's own inlier set (the returned mask stays the fp32 winner's, by contract)
        e = scene.src.astype(np.float64) @ ref["R"].astype(np.float64).T + ref["t"] - scene.tgt
        refit_mask = (e * e).sum(1) < cfg.tau ** 2
        assert (refit_mask & scene.inlier).sum() >= 0.95 * scene.inlier.sum()


def test_sharded_A_and_B_beyond_the_one_block_scans(pkg, O):
    """N > 8192: the row statistics and the row-count scans are separate launches again (two single-pass scans side by
    side in sharded mode, each with its own ticket word) — a configuration C0 .. C2 never reach.  World 1 (unsharded
    entry point), 2 and 3 on one context set reused across two scenes of different size."""
    import torch
    dev = torch.device("cuda:0")
    for n, seed in ((9000, 3), (8300, 4)):
        sc = pkg.synth.make_scene(n, 0.08, 3.0, 0.1, seed)
        kw = dict(sigma=0.1, t_cmp=0.9, tau=0.1, min_len=0.1, max_triangles=6000, rank_mode=0)
        ref = O.register(sc.src, sc.tgt, threads=8, **kw)
        d_src = torch.from_numpy(sc.src).to(dev); d_tgt = torch.from_numpy(sc.tgt).to(dev)
        for world in (1, 2, 3):
            rc, st, Rt, mask, hdr = _run_sharded_ab(pkg, n, kw, d_src, d_tgt, world)
            assert rc == ref["rc"] == 0
            assert (st["edges"], st["best_rank"], st["best_count"], st["tri_kept"]) == (ref["edges"], ref["best_rank"], ref["best_count"], ref["t_eff"])
            assert np.array_equal(mask, ref["mask"])
            assert Rt.tobytes() == np.concatenate([ref["R"].ravel(), ref["t"]]).astype(np.float32).tobytes()


def test_sharded_candidate_blobs_too_small_are_detected_and_retried(pkg, O):
    """A candidate blob holds max(2T/world, 4096) << shard_cand_level entries.  Started far too small (negative level:
    1024 entries for T = 10 000 over 2 and 3 ranks), the merge must notice that a cut list could have mattered and every
    rank must report SC_ERETRY together; after enough retries the result is the unsharded one.  The native multi-device
    entry retries by itself."""
    import torch
    cfg, scene = pkg.synth.make_config_scene("C1")
    kw = cfg.params()
    ref = O.register(scene.src, scene.tgt, threads=8, **kw)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    for world in (2, 3):
        levels = []
        rc, st, Rt, mask, hdr = _run_sharded_ab(pkg, cfg.n, kw, d_src, d_tgt, world, level=-4, levels_out=levels)
        assert levels[0] > -4                                         # at least one SC_ERETRY happened
        assert rc == 0 and (st["best_rank"], st["best_count"], st["tri_kept"]) == (ref["best_rank"], ref["best_count"], ref["t_eff"])
        assert np.array_equal(mask, ref["mask"])
        assert Rt.tobytes() == np.concatenate([ref["R"].ravel(), ref["t"]]).astype(np.float32).tobytes()
    p_small = pkg.make_params(shard_cand_level=0, **dict(kw, max_triangles=40000))   # default level on a bigger T
    plan = pkg.shard_plan(pkg.make_params(shard_world=8, **dict(kw, max_triangles=40000)), cfg.n)
    assert plan.cand_bytes_per_rank == 256 + 20 * 10240                # max(2 * 40000 / 8, 4096) -> 10 240 entries
    assert pkg.shard_plan(p_small, cfg.n).cand_bytes_per_rank == 256 + 20 * 40960    # world 1: T rounded up


# ---------------------------------------------------------------------------------------------------------
# C2 by filter + exact fix-up (sc_filter.hip): every count must be the canonical fp32 kernel's / the oracle's
# ---------------------------------------------------------------------------------------------------------
def _hyps_near_truth(O, sc, T, seed):
    """T hypotheses: half from inlier triangles (many inliers, residuals spread around tau), half from random ones."""
    n = len(sc.src)
    rng = np.random.default_rng(seed)
    inl = np.nonzero(sc.inlier)[0]
    tri = np.sort(np.stack([rng.choice(inl if h % 2 else n, 3, replace=False) for h in range(T)]), axis=1).astype(np.uint32)
    return O.kabsch3(sc.src, sc.tgt, tri)


@pytest.mark.parametrize("n,T,scale", [(1300, 5000, 1.0), (5000, 2048, 1.0), (2049, 700, 1e4), (1000, 300, 1e-4), (40, 9, 1.0)])
def test_score_filter_counts_bit_exact(pkg, O, n, T, scale):
    """sc_debug.score_filter = 2 forces the matrix-pipe filter on inputs of any size: ragged windows and hypothesis
    counts, coordinates of very different magnitudes (the filter rescales by a power of two), hypotheses the filter
    refuses (non-finite entries, entries beyond 1.5, a huge translation) — all counted exactly as the oracle does."""
    reg = pkg.Registrar(0)
    sc = _scene(pkg, n, seed=n + 5)
    src = (sc.src * scale).astype(np.float32); tgt = (sc.tgt * scale).astype(np.float32)
    tau = np.float32(0.05 * scale)

    class S: pass
    s2 = S(); s2.src, s2.tgt, s2.inlier = src, tgt, sc.inlier
    Rt0 = _hyps_near_truth(O, s2, T, seed=n)
    if T > 100:
        Rt0[7, 4] = np.nan; Rt0[11, 9] = np.inf; Rt0[13, :9] *= 3.0; Rt0[17, 10] = 1e9 * scale; Rt0[19, 0] = -np.inf
    kw = _params(pkg, float(tau), T)
    cnt0 = O.score(src, tgt, Rt0, kw["tau"])
    for knobs in (dict(score_filter=2), dict(score_filter=2, filter_splits=1), dict(score_filter=2, filter_splits=8),
                  dict(score_filter=3), dict(score_filter=3, filter_splits=1), dict(score_filter=3, filter_splits=8),
                  dict(score_filter=1)):
        reg.set_debug(**knobs)
        cnt, key = reg.score(src, tgt, pkg.make_params(**kw), Rt0)
        assert np.array_equal(cnt, cnt0), knobs
        assert key == O.best_key(cnt0)
    assert cnt0.max() > (5 if n < 100 else 20)
    reg.close()


def test_score_filter_gives_up_exactly(pkg, O):
    """What the filter cannot bound it hands to the exact pass: (1) tau far below the resolution of the fp16 splits and
    (2) tau beyond the scaled range — every wave asks for a recount; (3) correspondences whose residual under EVERY
    hypothesis sits within 1e-5 of tau — every test is undecided, the waves' queues overflow; (4) a global queue of 256
    entries — the flushes fail.  Counts equal the oracle's each time."""
    reg = pkg.Registrar(0)
    n, T = 3000, 1024
    sc = _scene(pkg, n, seed=77)
    Rt0 = _hyps_near_truth(O, sc, T, seed=3)
    for flt in (2, 3):
        reg.set_debug(score_filter=flt)
        for tau in (1e-6, 60.0):
            kw = _params(pkg, tau, T)
            cnt, _ = reg.score(sc.src, sc.tgt, pkg.make_params(**kw), Rt0)
            assert np.array_equal(cnt, O.score(sc.src, sc.tgt, Rt0, kw["tau"])), (flt, tau)
    # (3) q = p + tau * u (1 + 1e-5 r): identity-like hypotheses see |residual| = tau up to 1e-5
    rng = np.random.default_rng(5)
    p = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    tau = 0.05
    q = (p.astype(np.float64) + tau * u * (1 + 1e-5 * rng.uniform(-1, 1, (n, 1)))).astype(np.float32)
    Rt1 = np.zeros((T, 12), dtype=np.float32); Rt1[:, [0, 4, 8]] = 1.0
    Rt1[:, 9:] = rng.uniform(-1e-7, 1e-7, (T, 3)).astype(np.float32)
    kw = _params(pkg, tau, T)
    ref = O.score(p, q, Rt1, kw["tau"])
    assert 0.2 * n < ref.mean() < 0.8 * n                       # the canonical chain decides them one way or the other
    # (gram_kappa_q4 = 1: the Gram filter without its cut — every workgroup walks every correspondence)
    for knobs in (dict(score_filter=2), dict(score_filter=2, filter_lds_queue=64), dict(score_filter=2, filter_queue_cap=256),
                  dict(score_filter=3), dict(score_filter=3, filter_lds_queue=64), dict(score_filter=3, filter_queue_cap=256),
                  dict(score_filter=3, gram_kappa_q4=1), dict(score_filter=3, gram_kappa_q4=1, filter_lds_queue=64),
                  dict(score_filter=3, gram_kappa_q4=1, filter_queue_cap=256)):
        reg.set_debug(**knobs)
        cnt, _ = reg.score(p, q, pkg.make_params(**kw), Rt1)
        assert np.array_equal(cnt, ref), knobs
    # (4) on an ordinary scene
    for flt, pers in ((2, 0), (3, 0), (3, 1)):
        reg.set_debug(score_filter=flt, filter_queue_cap=256, gram_kappa_q4=pers)
        kw = _params(pkg, 0.05, T)
        cnt, _ = reg.score(sc.src, sc.tgt, pkg.make_params(**kw), Rt0)
        assert np.array_equal(cnt, O.score(sc.src, sc.tgt, Rt0, kw["tau"])), (flt, pers)
    reg.close()


def test_register_with_the_filter_forced_small_and_sharded(pkg, O):
    """Whole path with the filter on a call it would not choose by size (C1), and with stage C sharded over 3 ranks."""
    import torch
    reg = pkg.Registrar(0)
    reg.set_debug(score_filter=2)
    cfg, scene = pkg.synth.make_config_scene("C1")
    _check_register(pkg, O, reg, scene, cfg.params())
    kw = cfg.params()
    ref = O.register(scene.src, scene.tgt, threads=8, **kw)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    world = 3
    d_keys = torch.zeros(2 * world, dtype=torch.int64, device=dev)
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(cfg.n, dtype=torch.uint8, device=dev)
    for r in range(world):
        p = pkg.make_params(shard_rank=r, shard_world=world, shard_block=256, **kw)
        reg.hypothesize_device(d_src.data_ptr(), d_tgt.data_ptr(), cfg.n, p, d_keys.data_ptr() + 16 * r)
    rc, st = reg.finalize_gathered_device(d_keys.data_ptr(), world, d_Rt.data_ptr(), d_mask.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and (st["best_rank"], st["best_count"]) == (ref["best_rank"], ref["best_count"])
    assert np.array_equal(d_mask.cpu().numpy(), ref["mask"])
    reg.close()


def test_score_filter_many_windows_and_wide_indices(pkg, O):
    """70 000 correspondences (69 windows, point indices beyond 16 bits, several grid splits) x 2048 hypotheses: 1.4e8 tests,
    so the filter is chosen by size; counts against the oracle."""
    reg = pkg.Registrar(0)
    n, T = 70_000, 2048
    sc = _scene(pkg, n, seed=12)
    Rt0 = _hyps_near_truth(O, sc, T, seed=8)
    kw = _params(pkg, 0.05, T)
    cnt0 = O.score(sc.src, sc.tgt, Rt0, kw["tau"], threads=8)
    cnt, key = reg.score(sc.src, sc.tgt, pkg.make_params(**kw), Rt0)
    assert np.array_equal(cnt, cnt0) and key == O.best_key(cnt0) and cnt0.max() > 1000
    reg.set_debug(filter_splits=7)
    cnt, _ = reg.score(sc.src, sc.tgt, pkg.make_params(**kw), Rt0)
    assert np.array_equal(cnt, cnt0)
    reg.close()


def test_score_filter_equals_fp32_kernel_on_random_scenes(pkg, O):
    """Property: on random scenes of random size, scale, tau and hypothesis quality the filtered counts equal the fp32
    kernel's (GPU against GPU: the fp32 kernel is pinned to the oracle elsewhere)."""
    reg_f = pkg.Registrar(0); reg_f.set_debug(score_filter=2)
    reg_g = pkg.Registrar(0); reg_g.set_debug(score_filter=3)
    reg_p = pkg.Registrar(0); reg_p.set_debug(score_filter=1)
    rng = np.random.default_rng(2024)
    undecided_seen = 0
    for it in range(40):
        n = int(rng.integers(3, 3000)); T = int(rng.integers(1, 600))
        scale = float(10.0 ** rng.uniform(-3, 3)); tau_rel = float(10.0 ** rng.uniform(-3.5, -0.3))
        p = (rng.uniform(-1, 1, (n, 3)) * scale).astype(np.float32)
        ang = rng.uniform(0, np.pi); ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        t = rng.uniform(-1, 1, 3) * scale
        q = (p.astype(np.float64) @ R.T + t + rng.normal(size=(n, 3)) * tau_rel * scale * 0.5)
        out = rng.random(n) < 0.5
        q[out] = rng.uniform(-2, 2, (int(out.sum()), 3)) * scale
        q = q.astype(np.float32)
        # hypotheses: the truth perturbed at the scale of tau, so that many residuals land near the threshold
        Rt = np.zeros((T, 12), dtype=np.float32)
        for h in range(T):
            dR = np.eye(3) + rng.normal(size=(3, 3)) * tau_rel * 0.3
            Rt[h, :9] = (dR @ R).astype(np.float32).ravel()
            Rt[h, 9:] = (t + rng.normal(size=3) * tau_rel * scale * 0.7).astype(np.float32)
        kw = _params(pkg, tau_rel * scale, T)
        c_f, k_f = reg_f.score(p, q, pkg.make_params(**kw), Rt)
        c_p, k_p = reg_p.score(p, q, pkg.make_params(**kw), Rt)
        c_g, k_g = reg_g.score(p, q, pkg.make_params(**kw), Rt)
        assert np.array_equal(c_f, c_p) and k_f == k_p, (it, n, T, scale, tau_rel)
        assert np.array_equal(c_g, c_p) and k_g == k_p, ("gram", it, n, T, scale, tau_rel)
        undecided_seen += int(c_p.max() > 0)
    assert undecided_seen > 10
    reg_f.close(); reg_p.close(); reg_g.close()


def test_score_keeps_the_fp32_kernel_when_tau_is_off_the_filters_scale(pkg, O):
    """A call big enough for the filter but with tau at 1e-5 of the scene's extent (or 100 x it): the staging kernel has
    told the host the coordinate maxima, the host keeps the fp32 kernel (the filter would hand every wave to the exact
    recount) — counts as the oracle's either way."""
    reg = pkg.Registrar(0)
    n, T = 70_000, 2048
    sc = _scene(pkg, n, seed=13)
    Rt0 = _hyps_near_truth(O, sc, T, seed=9)
    for tau in (1e-5, 100.0):
        kw = _params(pkg, tau, T)
        cnt0 = O.score(sc.src, sc.tgt, Rt0, kw["tau"], threads=8)
        for knobs in (dict(), dict(score_filter=2)):
            reg.set_debug(**knobs)
            cnt, key = reg.score(sc.src, sc.tgt, pkg.make_params(**kw), Rt0)
            assert np.array_equal(cnt, cnt0) and key == O.best_key(cnt0), (tau, knobs)
    reg.close()


# ---------------------------------------------------------------------------------------------------------
# the BASELINE shapes in full — every count, and the 8-rank sharded forms
# ---------------------------------------------------------------------------------------------------------
_ORACLE_REGISTER = {}


def _oracle_register(O, pkg, name):
    """O.register of a BASELINE config, once per session (C3 is ~4e9 scoring tests on the host)."""
    if name not in _ORACLE_REGISTER:
        cfg, scene = pkg.synth.make_config_scene(name)
        _ORACLE_REGISTER[name] = O.register(scene.src, scene.tgt, threads=min(O.max_threads(), 64), **cfg.params())
    return _ORACLE_REGISTER[name]


@pytest.mark.parametrize("name", ["C2", "C3", "C4"])
def test_score_every_count_of_the_real_top_T_at_the_baseline_shapes(pkg, O, name):
    """The C2 stage at the shapes the headline numbers are quoted on, with the hypotheses the path really scores there
    (Kabsch of the ranked top-T list) and default knobs (so the matrix-pipe filter + exact pass is what runs): ALL T
    counts against the CPU restatement — not only the winner's, which is all the whole-path tests can see.
    C2: 50 000 x 5000, C3: 200 000 x 20 000 (4e9 tests), C4: 500 000 x 5000."""
    cfg, scene = pkg.synth.make_config_scene(name)
    reg = pkg.Registrar(0)
    try:
        p = pkg.make_params(**cfg.params())
        tri, key, total, edges = reg.triangles(scene.src, scene.tgt, p)
        assert len(tri) == cfg.T
        threads = min(O.max_threads(), 64)
        Rt0 = O.kabsch3(scene.src, scene.tgt, tri, threads=threads)
        Rt = reg.kabsch(scene.src, scene.tgt, p, tri)
        assert nan_equal_bits(Rt, Rt0)
        cnt0 = O.score(scene.src, scene.tgt, Rt0, cfg.tau, threads=threads)
        cnt, k = reg.score(scene.src, scene.tgt, p, Rt0)
        bad = np.nonzero(cnt != cnt0)[0]
        assert bad.size == 0, (name, bad[:10], cnt[bad[:10]], cnt0[bad[:10]])
        assert k == O.best_key(cnt0)
        info = reg.debug_last()
        # the Gram filter is chosen at all three (since r04b also at C3, whose tau is 1 % of the clouds' extent: in the frame of
        # a reference hypothesis the cancelling terms are small where it matters), and most hypotheses and few correspondences
        # are near that frame
        print(name, "Gram cut:", {k: info[k] for k in info if k.startswith("gram_") or k.startswith("filter_")})
        # (recounts: groups of 8 hypotheses far from the frame whose shell is too wide for the filter — C3 has a few)
        assert info["c2_kernel"] == 2 and info["filter_undecided"] > 0, info
        assert info["filter_recounts"] <= 0.01 * info["filter_splits"] * info["gram_rows"] / 8, info
        assert info["gram_near_hyp"] > 0.5 * info["gram_rows"] and 0 < info["gram_near_corr"] < 0.4 * cfg.n, info
        # ... and each kernel forced: the linear filter, the Gram filter (with and without its cut), the
        # plain fp32 kernel (what sc_debug.score_filter = 1 and the truncated scores run)
        for flt, kern, pers in ((2, 1, 0), (3, 2, 0), (3, 2, 1), (3, 2, 64), (1, 0, 0)):
            reg.set_debug(score_filter=flt, gram_kappa_q4=pers)
            cnt1, k1 = reg.score(scene.src, scene.tgt, p, Rt0)
            bad = np.nonzero(cnt1 != cnt0)[0]
            assert bad.size == 0 and k1 == k, (name, flt, pers, bad[:10], cnt1[bad[:10]], cnt0[bad[:10]], reg.debug_last())
            assert reg.debug_last()["c2_kernel"] == kern
        ref = _oracle_register(O, pkg, name)
        best = 0xFFFFFFFF - (k & 0xFFFFFFFF)
        assert (best, int(cnt0[best])) == (ref["best_rank"], ref["best_count"])
    finally:
        reg.close()


@pytest.mark.parametrize("name", ["C3", "C4"])
def test_sharded_A_and_B_world_8_at_the_configs_it_exists_for(pkg, O, name):
    """BASELINE configs[3] and [4] in their specified form: 8 ranks, stages A, B and C sharded (phase API; the ranks share
    the exchange buffers on this one GPU), against the CPU restatement: winner, count, mask, (R,t), and the ranks' row
    ranges partition the enumeration.  N = 20 000 is also the size at which the look-back ticket aliasing fault of
    round 2 (fixed in 2fee6e3) occurred."""
    import torch
    cfg, scene = pkg.synth.make_config_scene(name)
    kw = cfg.params()
    ref = _oracle_register(O, pkg, name)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    levels = []
    rc, st, Rt, mask, hdr = _run_sharded_ab(pkg, cfg.n, kw, d_src, d_tgt, 8, levels_out=levels)
    assert rc == ref["rc"] == 0 and levels == [0]                       # no SC_ERETRY at the default blob size
    assert (st["edges"], st["best_rank"], st["best_count"], st["tri_kept"]) == (ref["edges"], ref["best_rank"], ref["best_count"], ref["t_eff"])
    assert np.array_equal(mask, ref["mask"])
    assert Rt.tobytes() == np.concatenate([ref["R"].ravel(), ref["t"]]).astype(np.float32).tobytes()
    assert int(hdr[:, 0].sum()) == st["tri_total"]
    share = hdr[:, 0].astype(np.float64) / hdr[:, 0].sum()
    assert share.max() < 2.0 / 8, share


# ---------------------------------------------------------------------------------------------------------
# in-range worst cases for the matrix-pipe filter (sc_debug.score_filter = 2)
# ---------------------------------------------------------------------------------------------------------
def _filter_eta(p, q, Rt, tau):
    """The filter's own scale s, shell half-width eta (in scaled units) and eta relative to tau — the formulas of
    score_filter_kernel / filter_tile_block, with the call-wide max |t| (a wave uses its own 8 hypotheses' max)."""
    pmax = float(np.abs(p).max()); qmax = float(np.abs(q).max())
    e = int(np.floor(np.log2(max(pmax, qmax))))
    s = 2.0 ** (8 - e)
    tmax = float(np.abs(Rt[:, 9:]).max())
    eta = (2.6 * pmax * s + qmax * s + tmax * s) / 65536.0
    return s, eta, eta / (s * tau), pmax * s, qmax * s, tmax * s


def _plant(p, Rt, tau, eta_rel, rng, ks=(0.5, 1.0, 2.0)):
    """q such that correspondence m sits at residual tau * (1 +- k * eta) under hypothesis m mod T (k cycling through
    `ks`, the sign alternating): q = R p + t - r u, computed in float64 from the fp32 values the kernels see, rounded
    once to fp32 (that rounding is ~eta / 100).  Returns q and the k of every correspondence."""
    n, T = len(p), len(Rt)
    h = np.arange(n) % T
    R = Rt[h, :9].astype(np.float64).reshape(n, 3, 3); t = Rt[h, 9:].astype(np.float64)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    k = np.asarray(ks)[(np.arange(n) // T) % len(ks)]
    sign = np.where((np.arange(n) // (T * len(ks))) % 2 == 0, 1.0, -1.0)
    r = tau * (1.0 + sign * k * eta_rel)
    q = np.einsum("nij,nj->ni", R, p.astype(np.float64)) + t - r[:, None] * u
    return q.astype(np.float32), k


def _check_filter_case(pkg, O, reg, p, q, Rt, tau, k, expect_fast=True):
    kw = _params(pkg, float(tau), len(Rt))
    cnt0 = O.score(p, q, Rt, kw["tau"], threads=4)
    reg.set_debug(score_filter=2, filter_queue_cap=1 << 22)   # (these scenes queue ~1 % of their tests: 10 x a real one)
    cnt, key = reg.score(p, q, pkg.make_params(**kw), Rt)
    info = reg.debug_last()
    bad = np.nonzero(cnt != cnt0)[0]
    assert bad.size == 0, (bad[:8], cnt[bad[:8]], cnt0[bad[:8]])
    assert key == O.best_key(cnt0)
    assert info["c2_kernel"] == 1
    if expect_fast:
        assert info["filter_recounts"] == 0, info                      # the filter itself decided: nothing was refused
        assert info["filter_undecided"] >= 0.9 * (k == 0.5).sum(), info  # ... and the planted shell tests really queued
    reg.set_debug(score_filter=3, filter_queue_cap=1 << 22)   # the Gram filter on the same inputs (it may refuse them: counts only)
    cntg, keyg = reg.score(p, q, pkg.make_params(**kw), Rt)
    badg = np.nonzero(cntg != cnt0)[0]
    assert badg.size == 0 and keyg == key, ("gram", badg[:8], cntg[badg[:8]], cnt0[badg[:8]], reg.debug_last())
    reg.set_debug(score_filter=1)
    cnt1, _ = reg.score(p, q, pkg.make_params(**kw), Rt)
    assert np.array_equal(cnt1, cnt0)
    return cnt0, info


def test_score_filter_adversarial_large_R_entries(pkg, O):
    """Every |R_ij| in [1.3, 1.5) with signs aligned with the points (all positive, points in the positive octant): the
    row sums reach ~4.4 of the 4.5 the error bound allows for, |R p| is as large as it can get against |p|."""
    reg = pkg.Registrar(0)
    rng = np.random.default_rng(11)
    n, T = 6144, 1024
    p = rng.uniform(0.35, 1.0, (n, 3)).astype(np.float32)
    R0 = rng.uniform(1.40, 1.49, (3, 3))
    Rt = np.zeros((T, 12), dtype=np.float32)
    Rt[:, :9] = np.clip(R0.ravel()[None, :] + rng.normal(size=(T, 9)) * 2e-3, 1.3, 1.4999).astype(np.float32)
    Rt[:, 9:] = (np.array([0.3, -0.2, 0.1]) + rng.normal(size=(T, 3)) * 5e-3).astype(np.float32)
    tau = 0.02
    q0 = np.einsum("ij,nj->ni", R0, p.astype(np.float64)) + np.array([0.3, -0.2, 0.1])
    s, eta, eta_rel, Ps, Qs, Ts = _filter_eta(p, q0, Rt, tau)
    q, k = _plant(p, Rt, tau, eta_rel, rng)
    assert np.abs(Rt[:, :9]).min() >= 1.3 and np.abs(Rt[:, :9]).max() < 1.5 and np.abs(Rt[:, :9]).reshape(T, 3, 3).sum(2).max() > 4.2
    assert eta_rel < 0.25 and Qs < 512 and Ps < 512
    cnt0, info = _check_filter_case(pkg, O, reg, p, q, Rt, tau, k)
    assert cnt0.max() >= 3
    reg.close()


def test_score_filter_adversarial_large_translation_and_cancellation(pkg, O):
    """|t| s in [1500, 2048) — as large as the filter accepts — which needs |R p| of the same size to land on a q inside
    the scaled range: R entries ~1.45, p near (-1.6, -1.6, -1.6): R p + t cancels from ~7 down to a cloud of extent
    ~0.5, the worst case for every rounding of both evaluations."""
    reg = pkg.Registrar(0)
    rng = np.random.default_rng(12)
    n, T = 6144, 1024
    R0 = rng.uniform(1.36, 1.49, (3, 3))
    p0 = np.array([-1.7, -1.5, -1.6])
    t0 = -R0 @ p0                                              # R0 p0 + t0 = 0: components ~ 6.9
    p = (p0[None, :] + rng.uniform(-0.06, 0.06, (n, 3))).astype(np.float32)
    assert 1.0 < np.abs(p).max() < 2.0                         # s = 256
    Rt = np.zeros((T, 12), dtype=np.float32)
    Rt[:, :9] = np.clip(R0.ravel()[None, :] + rng.normal(size=(T, 9)) * 1e-3, 1.3, 1.4999).astype(np.float32)
    Rt[:, 9:] = (t0 + rng.normal(size=(T, 3)) * 3e-3).astype(np.float32)
    tau = 0.02
    q0 = np.einsum("ij,nj->ni", R0, p.astype(np.float64)) + t0
    s, eta, eta_rel, Ps, Qs, Ts = _filter_eta(p, q0, Rt, tau)
    assert s == 256.0 and 1500.0 <= Ts < 2048.0 and eta_rel < 0.25
    q, k = _plant(p, Rt, tau, eta_rel, rng)
    cnt0, info = _check_filter_case(pkg, O, reg, p, q, Rt, tau, k)
    assert cnt0.max() >= 3
    reg.close()


def test_score_filter_adversarial_large_tau_and_translation(pkg, O):
    """tau itself near the top of the filter's range (s tau ~ 3100 of 4096) with |t| ~ tau: proper rotations, a small
    cloud, every residual about |t| — the shell sits at the far end of the scaled range."""
    reg = pkg.Registrar(0)
    rng = np.random.default_rng(13)
    n, T = 6144, 1024
    p = rng.uniform(-1.3, 1.3, (n, 3)).astype(np.float32)
    p[0] = (1.5, -1.5, 1.5)
    t0 = np.array([7.0, -6.5, 7.5])
    Rt = np.zeros((T, 12), dtype=np.float32)
    for h in range(T):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(0, 0.02)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rt[h, :9] = (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K).astype(np.float32).ravel()
    Rt[:, 9:] = (t0 + rng.normal(size=(T, 3)) * 2e-2).astype(np.float32)
    tau = float(np.linalg.norm(t0))                            # 12.13: s tau = 3106
    # planted: q = R p + t - r u with u ~ t / |t| (+ a little spread), so that q stays a small cloud
    h = np.arange(n) % T
    R = Rt[h, :9].astype(np.float64).reshape(n, 3, 3); t = Rt[h, 9:].astype(np.float64)
    u = t0 / np.linalg.norm(t0) + rng.normal(size=(n, 3)) * 0.01
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    s, eta, eta_rel, Ps, Qs, Ts = _filter_eta(p, p, Rt, tau)
    k = np.asarray((0.5, 1.0, 2.0))[(np.arange(n) // T) % 3]
    sign = np.where((np.arange(n) // (3 * T)) % 2 == 0, 1.0, -1.0)
    r = tau * (1.0 + sign * k * eta_rel)
    q = (np.einsum("nij,nj->ni", R, p.astype(np.float64)) + t - r[:, None] * u).astype(np.float32)
    s2, eta2, eta_rel2, Ps, Qs, Ts = _filter_eta(p, q, Rt, tau)
    assert s2 == s == 256.0 and Qs < 512 and 2048 < s * tau <= 4096 and Ts <= 2048 and abs(eta2 - eta) < 0.1 * eta
    cnt0, info = _check_filter_case(pkg, O, reg, p, q, Rt, tau, k)
    assert 0.2 * n < cnt0.mean() < 0.8 * n                     # every hypothesis sees about every residual near tau
    reg.close()


@pytest.mark.parametrize("flat", [1e-6, 3e-5])
def test_score_filter_adversarial_near_planar_cloud(pkg, O, flat):
    """One coordinate `flat` times the others (a near-planar cloud, both sides): its scaled values sit at 5e-4 .. 1.5e-2,
    so the fp16 low halves of the split are sub-normal (or flush to zero in the matrix pipe) — the case the bound's
    comment only estimates."""
    reg = pkg.Registrar(0)
    rng = np.random.default_rng(14)
    n, T = 6144, 1024
    p = rng.uniform(-1.0, 1.0, (n, 3)); p[:, 2] *= flat
    p = p.astype(np.float32)
    Rt = np.zeros((T, 12), dtype=np.float32)
    for h in range(T):
        ang = 0.7 + rng.normal() * 2e-3; c, s_ = np.cos(ang), np.sin(ang)
        N = rng.normal(size=(3, 3)) * 1e-4; N[2, :2] *= flat          # (nothing may lift the cloud out of its plane)
        Rz = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1.0]]) + N
        Rt[h, :9] = Rz.astype(np.float32).ravel()
    Rt[:, 9:] = (np.array([0.2, -0.1, 0.0]) + rng.normal(size=(T, 3)) * np.array([4e-3, 4e-3, 4e-3 * flat])).astype(np.float32)
    tau = 0.01
    s, eta, eta_rel, Ps, Qs, Ts = _filter_eta(p, p * 1.3, Rt, tau)
    # planted in the plane (u_z scaled like the cloud), so that q stays near-planar too
    h = np.arange(n) % T
    R = Rt[h, :9].astype(np.float64).reshape(n, 3, 3); t = Rt[h, 9:].astype(np.float64)
    u = rng.normal(size=(n, 3)); u[:, 2] *= flat; u /= np.linalg.norm(u, axis=1, keepdims=True)
    k = np.asarray((0.5, 1.0, 2.0))[(np.arange(n) // T) % 3]
    sign = np.where((np.arange(n) // (3 * T)) % 2 == 0, 1.0, -1.0)
    r = tau * (1.0 + sign * k * eta_rel)
    q = (np.einsum("nij,nj->ni", R, p.astype(np.float64)) + t - r[:, None] * u).astype(np.float32)
    assert np.abs(q[:, 2]).max() < 20 * flat
    s2, eta2, eta_rel2, Ps, Qs, Ts = _filter_eta(p, q, Rt, tau)
    assert s2 == s and abs(eta2 - eta) < 0.25 * eta
    cnt0, info = _check_filter_case(pkg, O, reg, p, q, Rt, tau, k)
    reg.close()


def test_score_filter_adversarial_one_far_outlier_sets_the_scale(pkg, O):
    """A single correspondence 150 x further out than the cloud sets the power-of-two scale: the cloud's scaled
    coordinates drop to ~2, its fp16 low halves to 1e-3 — and tau, still in range, is only ~6 eta."""
    reg = pkg.Registrar(0)
    rng = np.random.default_rng(15)
    n, T = 6144, 1024
    p = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    p[n - 1] = (150.0, -20.0, 30.0)
    Rt = np.zeros((T, 12), dtype=np.float32)
    ax = np.array([0.3, -0.5, 0.8]); ax /= np.linalg.norm(ax)
    for h in range(T):
        ang = 1.1 + rng.normal() * 0.3                    # (hypotheses far apart against tau: the shell is 9 % of tau wide here)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rt[h, :9] = (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K).astype(np.float32).ravel()
    Rt[:, 9:] = (np.array([0.1, 0.2, -0.3]) + rng.normal(size=(T, 3)) * 0.5).astype(np.float32)
    tau = 0.1
    q0 = np.einsum("ij,nj->ni", Rt[0, :9].astype(np.float64).reshape(3, 3), p.astype(np.float64)) + Rt[0, 9:]
    s, eta, eta_rel, Ps, Qs, Ts = _filter_eta(p, q0, Rt, tau)
    assert s <= 2.0 and eta_rel < 0.25, (s, eta_rel)
    q, k = _plant(p, Rt, tau, eta_rel, rng)
    s2, eta2, _, Ps, Qs, Ts = _filter_eta(p, q, Rt, tau)
    assert s2 == s and Qs < 512
    cnt0, info = _check_filter_case(pkg, O, reg, p, q, Rt, tau, k)
    assert cnt0.max() >= 3
    reg.close()


def test_score_kernel_choice_without_the_maxima(pkg, O):
    """The host decides ONCE per call which C2 kernel runs (sc_capi.hip decide_filter) from the coordinate maxima the
    staging kernel publishes; sc_debug.filter_blind makes it decide as if they had not arrived: it then assumes the
    filter applies, and with tau off the filter's scale every wave hands its work to the exact recount — same counts.
    With the maxima (the default; the stage hook waits for them) the same call keeps the plain kernel."""
    reg = pkg.Registrar(0)
    n, T = 70_000, 2048
    sc = _scene(pkg, n, seed=13)
    Rt0 = _hyps_near_truth(O, sc, T, seed=9)
    kw = _params(pkg, 1e-5, T)
    cnt0 = O.score(sc.src, sc.tgt, Rt0, kw["tau"], threads=8)
    cnt, _ = reg.score(sc.src, sc.tgt, pkg.make_params(**kw), Rt0)
    assert np.array_equal(cnt, cnt0) and reg.debug_last()["c2_kernel"] == 0
    reg.set_debug(filter_blind=1)
    cnt, _ = reg.score(sc.src, sc.tgt, pkg.make_params(**kw), Rt0)
    info = reg.debug_last()
    assert np.array_equal(cnt, cnt0) and info["c2_kernel"] == 1 and info["filter_recounts"] == T // 8 * info["filter_splits"], info
    reg.close()


def _unshuffled(scene):
    """The same scene with its correspondences reordered so that the true inliers come first (a correspondence list in
    keypoint order: inliers cluster in index), everything else in the original order."""
    order = np.argsort(~scene.inlier, kind="stable")

    class S: pass
    s = S()
    s.src = np.ascontiguousarray(scene.src[order]); s.tgt = np.ascontiguousarray(scene.tgt[order])
    s.inlier = scene.inlier[order]; s.R_gt, s.t_gt = scene.R_gt, scene.t_gt
    return s


@pytest.mark.parametrize("name,world", [("C2", 8), ("C1", 4)])
def test_sharded_A_and_B_balance_on_an_unshuffled_scene(pkg, O, name, world):
    """correspondence lists come in keypoint order, so the inliers — and with them nearly all the
    triangles of the pruned graph — sit in a few rows.  The ranks' row ranges are cut by the work of the PRUNED graph
    (strong edges per row, known after the certificate), so that every rank still enumerates about the same share and
    its share of the global top-T fits the default candidate blob: no SC_ERETRY at level 0, max / mean enumerated per
    rank below 1.3, and the result is the oracle's."""
    import torch
    cfg, scene0 = pkg.synth.make_config_scene(name)
    scene = _unshuffled(scene0)
    kw = cfg.params()
    ref = O.register(scene.src, scene.tgt, threads=8, **kw)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(scene.src).to(dev); d_tgt = torch.from_numpy(scene.tgt).to(dev)
    levels = []
    rc, st, Rt, mask, hdr = _run_sharded_ab(pkg, cfg.n, kw, d_src, d_tgt, world, levels_out=levels)
    assert rc == ref["rc"] == 0 and levels == [0], levels
    assert (st["edges"], st["best_rank"], st["best_count"], st["tri_kept"]) == (ref["edges"], ref["best_rank"], ref["best_count"], ref["t_eff"])
    assert np.array_equal(mask, ref["mask"])
    assert Rt.tobytes() == np.concatenate([ref["R"].ravel(), ref["t"]]).astype(np.float32).tobytes()
    enum = hdr[:, 0].astype(np.float64)
    assert int(enum.sum()) == st["tri_total"]
    assert enum.max() / enum.mean() < 1.3, enum


# ---------------------------------------------------------------------------------------------------------
# timing flags: diagnostics only — they must not change a result, and what they report must be sane
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score_filter", [1, 2, 3])
def test_timing_flags_change_nothing_and_report_sane_times(pkg, reg, score_filter):
    """SC_FLAG_TIMING (every stage bracketed by event records, speculative launches off), SC_FLAG_TIMING_HOT (the score
    stage from the dispatch packets of its own kernels: what bench.py's `roofline` is made of) and SC_FLAG_TIMING_ONE (one
    bracket on the hot path) — for each of the three stage-C2 kernels: same winner, mask and (R, t) as the untimed call;
    the hot figure agrees with the fully bracketed one; every single bracket is positive and below the call's wall time."""
    cfg, scene = pkg.synth.make_config_scene("C1")
    reg.set_debug(score_filter=score_filter)
    base = reg.register(scene.src, scene.tgt, **cfg.params())
    assert reg.debug_last()["c2_kernel"] == score_filter - 1
    full = reg.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_TIMING, **cfg.params())
    hot = reg.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_TIMING_HOT, **cfg.params())
    for got in (full, hot):
        assert got["stats"]["best_rank"] == base["stats"]["best_rank"] and got["stats"]["best_count"] == base["stats"]["best_count"]
        assert np.array_equal(got["mask"], base["mask"]) and nan_equal_bits(got["R"], base["R"]) and nan_equal_bits(got["t"], base["t"])
    us_full, us_hot = full["stats"]["us_score"], hot["stats"]["us_score"]
    assert 1.0 < us_hot < 5000.0 and 1.0 < us_full < 5000.0
    assert 0.4 < us_hot / us_full < 2.5, (us_hot, us_full)   # two clocks around the same kernels
    assert hot["stats"]["us_compat"] == 0.0                  # only the hot bracket is taken
    names = ["us_stage", "us_compat", "us_triangles", "us_kabsch", "us_score", "us_argmax", "us_mask"]
    for k, name in enumerate(names):
        one = reg.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_TIMING_ONE | pkg.SC_TIMING_STAGE(k), **cfg.params())
        assert one["stats"]["best_rank"] == base["stats"]["best_rank"] and np.array_equal(one["mask"], base["mask"])
        assert 0.0 < one["stats"][name] < 5000.0, (name, one["stats"][name])
        assert all(one["stats"][o] == 0.0 for o in names if o != name)
    reg.set_debug()
