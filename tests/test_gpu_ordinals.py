"""GPU: stage B's ordinals from the ORDERED strong list (sc_tri.hip 2c) — no scan launch between the counting pass and the key kernel.

A triangle's ordinal is (triangles of the earlier edges, in edge order) + (its rank inside its edge); ties at the T-th key are cut by
it.  The hot path (event list, a-priori select window, a context that already holds key arrays) now takes it from the pruning
kernel's ordered list, chunk totals and the key kernel's own prefix instead of a scan over every edge's count.  Everything must
stay bit for bit: the ranked list against the CPU restatement, the new form against the scan form (sc_debug.scan_ordinals), the two
overflow fall-backs, and host-free frames whose launches cover more edges than the graph has.  Shapes are a few hundred
correspondences: just enough edges (>= 4096) for the pruned event path.
"""
import numpy as np
import pytest

from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu


def _params(tau, T, **kw):
    d = dict(sigma=tau, t_cmp=0.9, tau=tau, min_len=tau, max_triangles=T, rank_mode=0)
    d.update(kw)
    return d


def _clique_scene(m, n_out=150, eps=0.03, seed=3):
    """`m` correspondences that move rigidly and exactly (every edge among them weighs 1.0f, every triangle's key is 3.0f), far away
    from `n_out` correspondences of a scaled scene q = (1 + eps) p, whose edges weigh exp(-(eps len)^2 / 2 sigma^2) <= 0.9952 from
    min_len up; no edge between the two groups (the residual there is >= eps, beyond the threshold 0.7 eps).  With T below the
    clique's C(m, 3) triangles the pruning bound lands in the top histogram bin and the strong edges are the clique's C(m, 2)."""
    rng = np.random.default_rng(seed)
    out = rng.uniform([1.0, -0.5, -0.5], [2.0, 0.5, 0.5], (n_out, 3)).astype(np.float32)
    cl = (np.array([50.0, 0.0, 0.0]) + rng.uniform(-0.5, 0.5, (m, 3))).astype(np.float32)
    n = n_out + m
    src = np.empty((n, 3), np.float32); tgt = np.empty((n, 3), np.float32)
    is_cl = np.zeros(n, bool); is_cl[np.arange(m) * (n // m) + 5] = True   # spread over the rows: the clique's edges are far apart in edge order
    src[is_cl] = cl; tgt[is_cl] = cl
    src[~is_cl] = out; tgt[~is_cl] = (out * np.float32(1.0 + eps)).astype(np.float32)
    sigma = eps * 0.7 / 0.459
    return src, tgt, dict(sigma=sigma, t_cmp=0.9, tau=sigma, min_len=0.15, rank_mode=0)


class _Scenes:
    """The scenes of this file and the CPU restatement's ranked lists for them, computed once."""

    def __init__(self, pkg, O):
        ties = pkg.synth.make_scene(150, 1.0, 1.0, 1e-7, 21)          # noise-free, all inliers: one key value, E = 11 167
        plain = pkg.synth.make_scene(300, 0.3, 1.0, 0.05, 7)           # E = 4401, 42 316 triangles, practically no ties
        c8 = _clique_scene(8); c12 = _clique_scene(12)
        self.cases = {
            "ties": (ties.src, ties.tgt, _params(0.05, 3000)),
            "plain": (plain.src, plain.tgt, _params(0.05, 1000)),
            "clique8": (c8[0], c8[1], dict(c8[2], max_triangles=30)),      # 28 strong edges: less than one chunk
            "clique12": (c12[0], c12[1], dict(c12[2], max_triangles=100)), # 66 strong edges: chunks of 16, 32 or 64 never divide it
        }
        self.ref = {}
        for name, (src, tgt, kw) in self.cases.items():
            S0, bits0, deg0 = O.compat(src, tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"])
            T = kw["max_triangles"]
            tri0, key0, total0 = O.triangles(S0, bits0, deg0, T + 64, 0)   # 64 more: what lies just beyond the T-th place
            self.ref[name] = dict(tri=tri0[:T], key=key0[:T], beyond=key0[T:], total=total0, edges=int(deg0.sum()) // 2)


@pytest.fixture(scope="module")
def scenes(pkg, O):
    return _Scenes(pkg, O)


@pytest.fixture()
def warm(pkg, scenes):
    """A context that holds key arrays (the new form rides the speculative key pass, which a context's first call cannot take)."""
    r = pkg.Registrar(0)
    src, tgt, kw = scenes.cases["plain"]
    r.triangles(src, tgt, pkg.make_params(**kw))
    yield r
    r.close()


def _ranked(pkg, r, scenes, name):
    src, tgt, kw = scenes.cases[name]
    tri, key, total, edges = r.triangles(src, tgt, pkg.make_params(**kw))
    return tri, key, total, edges, r.debug_last()


def _check_ranked(scenes, name, got):
    tri, key, total, edges, _ = got
    ref = scenes.ref[name]
    assert (total, edges) == (ref["total"], ref["edges"])
    assert np.array_equal(key, ref["key"]), f"{name}: keys differ from the CPU restatement"
    assert np.array_equal(tri, ref["tri"]), f"{name}: triangles or their order differ from the CPU restatement"


def test_the_test_scenes_put_equal_keys_across_the_T_th_place(scenes):
    """Without keys that tie across the cut the comparisons below would prove nothing about ordinals."""
    for name in ("ties", "clique8", "clique12"):
        ref = scenes.ref[name]
        k = ref["key"][-1]
        inside, beyond = int((ref["key"] == k).sum()), int((ref["beyond"] == k).sum())
        assert inside >= 5 and beyond >= 5, (name, inside, beyond)
    assert scenes.ref["ties"]["total"] > 100_000 and len(np.unique(scenes.ref["ties"]["key"])) == 1
    assert min(r["edges"] for r in scenes.ref.values()) >= 4096   # the pruned event path


@pytest.mark.parametrize("name", ["ties", "plain", "clique8", "clique12"])
def test_ranked_list_equals_the_cpu_restatement(pkg, scenes, warm, name):
    got = _ranked(pkg, warm, scenes, name)
    assert got[4]["ordinals"] == 1, got[4]
    _check_ranked(scenes, name, got)


@pytest.mark.parametrize("tg", [4, 8, 16])
@pytest.mark.parametrize("cnt_blocks", [1, 3, 0])
def test_chunk_edges(pkg, scenes, warm, cnt_blocks, tg):
    """One workgroup (as many trips as chunks), three (odd strides), the default grid (one trip); chunks of 64, 32 and 16 positions;
    lists shorter than a chunk, of a length no chunk divides, and of several hundred chunks."""
    warm.set_debug(cnt_blocks=cnt_blocks, tg_events=tg)
    chunk = 256 // tg
    seen = {}
    for name in ("clique8", "clique12", "plain", "ties"):
        got = _ranked(pkg, warm, scenes, name)
        assert got[4]["ordinals"] == 1, (name, got[4])
        _check_ranked(scenes, name, got)
        seen[name] = got[4]["strong_edges"]
    print(f"strong edges (cnt_blocks={cnt_blocks}, tg_events={tg}): {seen}")
    assert 3 <= seen["clique8"] < 64 and seen["clique8"] % chunk != 0  # below 64: one chunk of 64 or 32 positions, two of 16
    assert seen["clique12"] > 64 and seen["clique12"] % 16 != 0        # two chunks or more, the last one partial
    assert seen["plain"] > 4 * chunk and seen["plain"] % chunk != 0    # several chunks
    assert seen["ties"] > 100 * chunk and seen["ties"] % chunk != 0    # more trips than one even on the default grid's 256 workgroups at 16 positions


def _register(r, scene_case, **extra):
    src, tgt, kw = scene_case
    out = r.register(src, tgt, **dict(kw, **extra))
    return out, r.debug_last()


@pytest.mark.parametrize("name", ["ties", "plain", "clique12"])
def test_new_form_equals_scan_form(pkg, scenes, name):
    """sc_debug.scan_ordinals keeps the scan on the same binary: the ranked list, sc_register's outputs and the edge count are equal,
    and sc_debug_last says which form ran."""
    res = {}
    for scan in (0, 1):
        r = pkg.Registrar(0)
        try:
            if scan:
                r.set_debug(scan_ordinals=1)
            _register(r, scenes.cases[name])                           # (the context's first call: no key arrays yet)
            out, info = _register(r, scenes.cases[name])
            assert info["ordinals"] == (0 if scan else 1), info
            lst = _ranked(pkg, r, scenes, name)
            assert lst[4]["ordinals"] == (0 if scan else 1), lst[4]
            res[scan] = (out, lst)
        finally:
            r.close()
    (a, la), (b, lb) = res[0], res[1]
    assert a["status"] == b["status"] == 0
    assert a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes() and np.array_equal(a["mask"], b["mask"])
    for k in ("best_rank", "best_count", "tri_total", "tri_kept", "edges"):
        assert a["stats"][k] == b["stats"][k], k
    assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]) and la[2:4] == lb[2:4]
    _check_ranked(scenes, name, la)


@pytest.mark.parametrize("name,knob", [("ties", dict(event_cap=4096)), ("plain", dict(event_cap=1024)),   # (`plain` records fewer than 4096 events)
                                       ("ties", dict(ord_chunk_max=2)), ("plain", dict(ord_chunk_max=2))])
def test_overflows_fall_back_through_the_scan(pkg, O, scenes, warm, name, knob):
    """An event region that is full, or more chunks than the key kernel is told to hold: the call walks the rows again, which needs
    the scan's offsets — the scan runs after all, over counts whose weak entries the ordered form never wrote.  After a chunk
    overflow the context keeps the scan form (the same graph would overflow again) until sc_set_debug resets it."""
    src, tgt, kw = scenes.cases[name]
    ref = O.register(src, tgt, threads=4, **kw)
    warm.set_debug(**knob)
    got = _ranked(pkg, warm, scenes, name)
    assert got[4]["ordinals"] == 2, got[4]
    _check_ranked(scenes, name, got)
    out, info = _register(warm, scenes.cases[name])
    assert info["ordinals"] == (0 if "ord_chunk_max" in knob else 2), info
    assert out["status"] == ref["rc"] == 0
    assert (out["stats"]["edges"], out["stats"]["best_rank"], out["stats"]["best_count"]) == (ref["edges"], ref["best_rank"], ref["best_count"])
    assert np.array_equal(out["mask"], ref["mask"]) and nan_equal_bits(out["R"], ref["R"]) and nan_equal_bits(out["t"], ref["t"])
    warm.set_debug()
    got = _ranked(pkg, warm, scenes, name)
    assert got[4]["ordinals"] == 1, got[4]
    _check_ranked(scenes, name, got)


def test_host_free_frames_whose_cover_exceeds_the_live_edges(pkg):
    """Two contexts, frames in flight on both, ten distinct scenes of one shape whose edge counts differ by more than 1.5 x: a
    host-free frame's launches cover the largest recent count, so the pruning kernel's workgroups beyond the live edges leave
    early and their counts must not be read.  Every frame equals the waited call on its scene bit for bit."""
    import torch
    dev = torch.device("cuda:0")
    n, frames, passes = 400, 10, 3
    rhos = [0.30, 0.50, 0.34, 0.46, 0.32, 0.42, 0.36, 0.48, 0.31, 0.40]
    scs = [pkg.synth.make_scene(n, rhos[k], 1.0, 0.05, 100 + k) for k in range(frames)]
    p = pkg.make_params(**_params(0.05, 2000))
    ds = [torch.from_numpy(s.src).to(dev) for s in scs]
    dt = [torch.from_numpy(s.tgt).to(dev) for s in scs]
    # the waited call on every scene (sc_debug.no_fast), scan form: the reference
    want = []
    w = pkg.Registrar(0)
    try:
        w.set_debug(no_fast=1, scan_ordinals=1)
        Rt1 = torch.zeros(12, dtype=torch.float32, device=dev); m1 = torch.zeros(n, dtype=torch.uint8, device=dev)
        for k in range(frames):
            rc, st = w.register_device(ds[k].data_ptr(), dt[k].data_ptr(), n, p, Rt1.data_ptr(), m1.data_ptr())
            assert rc == 0 and w.debug_last()["ordinals"] == 0
            want.append((st, Rt1.cpu().numpy().copy(), m1.cpu().numpy().copy()))
    finally:
        w.close()
    edges = [st["edges"] for st, _, _ in want]
    assert min(edges) >= 4096 and max(edges) >= 1.5 * min(edges), edges
    total = passes * frames
    Rt = torch.zeros(total, 12, dtype=torch.float32, device=dev)
    mask = torch.full((total, n), 7, dtype=torch.uint8, device=dev)
    pair = [pkg.Registrar(0), pkg.Registrar(0)]
    try:
        for g in pair:
            g.set_stream(torch.cuda.current_stream().cuda_stream)
        stats = []
        pair[0].register_device_async(ds[0].data_ptr(), dt[0].data_ptr(), n, p, Rt[0].data_ptr(), mask[0].data_ptr())
        for f in range(1, total + 1):
            if f < total:
                k = f % frames
                pair[f & 1].register_device_async(ds[k].data_ptr(), dt[k].data_ptr(), n, p, Rt[f].data_ptr(), mask[f].data_ptr())
            stats.append(pair[(f - 1) & 1].wait())
        torch.cuda.synchronize()
        # the repeated shape: one more frame on each context, the scene with the FEWEST edges under a cover sized by the largest
        k_min = int(np.argmin(edges))
        last = []
        for g in pair:
            rc, st = g.register_device(ds[k_min].data_ptr(), dt[k_min].data_ptr(), n, p, Rt1.data_ptr(), m1.data_ptr())
            info = g.debug_last()
            last.append((rc, st, Rt1.cpu().numpy().copy(), m1.cpu().numpy().copy(), info))
    finally:
        for g in pair:
            g.close()
    got_Rt, got_mask = Rt.cpu().numpy(), mask.cpu().numpy()
    for f, (rc, st) in enumerate(stats):
        st0, Rt0, m0 = want[f % frames]
        assert rc == 0, (f, rc)
        for key in ("edges", "tri_total", "tri_kept", "best_rank", "best_count"):
            assert st[key] == st0[key], (f, key, st[key], st0[key])
        assert got_Rt[f].tobytes() == Rt0.tobytes(), f"frame {f}: (R, t) differs from the waited call"
        assert np.array_equal(got_mask[f], m0), f"frame {f}: the mask differs from the waited call"
    for rc, st, Rt_l, m_l, info in last:
        st0, Rt0, m0 = want[k_min]
        assert rc == 0 and Rt_l.tobytes() == Rt0.tobytes() and np.array_equal(m_l, m0)
        assert info["fast_path"] == 1 and info["ordinals"] == 1, info
        assert info["cover_edges"] >= 1.5 * edges[k_min], (info, edges)   # the cover really exceeds the live edges
        assert info["n_hostfree_grow"] == 0, info
        assert info["n_fast_ok"] >= frames, info    # (of 16 frames per context: at worst the first pass waited or was repeated)
