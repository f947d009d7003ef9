"""GPU: refits iterated to a fixed point on a scored frame (include/saccot.h, sc_polish / sc_polish_device).

The expected value of every case is tests/polish_ref.py — the semantics restated on the CPU restatement's O.score / O.mask /
O.refine — and everything is compared bit for bit: every field of every candidate record, the winner's (R, t), the mask,
best_rank and best_count.

The scenes here are the configs' own (unit scale).  tests/test_gpu_polish_range.py runs the iterated refit, its candidate select and
its stop rules at the ends of the fp32 range.
"""
import ctypes as C

import numpy as np
import pytest

import polish_ref
from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
SC_FLAG_REFINE = 8


def _threads(O):
    return min(O.max_threads(), 16)


_HYP = {}


def _hyp(O, tag, src, tgt, kw):
    """Stage A -> ranked list -> Kabsch on the CPU, once per scene and session (the hypotheses do not depend on tau or the score mode)."""
    if tag not in _HYP:
        _HYP[tag] = polish_ref.hypotheses(O, src, tgt, kw, _threads(O))
    return _HYP[tag]


_REF = {}


def _ref(O, tag, src, tgt, kw, k, iters, mode=0):
    key = (tag, kw["tau"], mode, k, iters)
    if key not in _REF:
        _REF[key] = polish_ref.polish(O, src, tgt, _hyp(O, tag, src, tgt, kw)["Rt"], kw["tau"], mode, k, iters, threads=_threads(O))
    return _REF[key]


def _config(pkg, name):
    cfg, sc = pkg.synth.make_config_scene(name)
    return cfg.params(), sc.src, sc.tgt


def _flat(res):
    return np.concatenate([res["R"].ravel(), res["t"]])


def _assert_polish(got, exp, k, what=""):
    print(what, "status", got["status"], "n_cand", got["n_cand"], "rank", got["stats"]["best_rank"], "count", got["stats"]["best_count"],
          "| expected", exp["status"], len(exp["cand"]), exp["best_rank"], exp["best_count"],
          "iters", [int(c["iters"]) for c in got["cand"][: got["n_cand"]]], "|", [c["iters"] for c in exp["cand"]])
    assert got["status"] == exp["status"], what
    assert got["n_cand"] == len(exp["cand"]) and len(got["cand"]) == k, what
    for i, e in enumerate(exp["cand"]):
        g = got["cand"][i]
        assert (int(g["rank"]), int(g["score0"]), int(g["score"]), int(g["iters"]), int(g["reserved"])) == \
            (e["rank"], e["score0"], e["score"], e["iters"], 0), (what, i)
        assert nan_equal_bits(g["Rt"], e["Rt"]), (what, i)
    assert got["cand"][got["n_cand"]:].tobytes() == bytes(64 * (k - got["n_cand"])), what  # past K: zeroed
    assert nan_equal_bits(_flat(got), exp["Rt"]), what
    assert np.array_equal(got["mask"], exp["mask"]), what
    assert got["stats"]["best_rank"] == exp["best_rank"] and got["stats"]["best_count"] == exp["best_count"], what


def _same_polish(a, b, what=""):
    assert a["status"] == b["status"] and a["n_cand"] == b["n_cand"], what
    assert a["cand"].tobytes() == b["cand"].tobytes() and _flat(a).tobytes() == _flat(b).tobytes(), what
    assert np.array_equal(a["mask"], b["mask"]), what
    assert all(a["stats"][f] == b["stats"][f] for f in ("n", "edges", "tri_total", "tri_kept", "tri_scored", "best_rank", "best_count")), what


def _frame(r, pkg, src, tgt, kw, **extra):
    f = r.register(src, tgt, params=pkg.make_params(**kw, **extra))
    assert f["status"] == SC_OK
    return f


# ---- 1: the configs' own scenes, one and eight candidates, one and sixteen refits ------------------------------------------
@pytest.mark.parametrize("name", ["C0", "C1"])  # C0: n = 500, 8 chunks, the last of 52
def test_polish_equals_the_reference(pkg, O, reg, name):
    kw, src, tgt = _config(pkg, name)
    f = _frame(reg, pkg, src, tgt, kw)
    for k in (1, 8):
        for iters in (1, 16):
            got = reg.polish(candidates=k, max_iter=iters)
            _assert_polish(got, _ref(O, name, src, tgt, kw, k, iters), k, f"{name} K={k} max_iter={iters}")
            assert all(got["stats"][x] == f["stats"][x] for x in ("n", "edges", "tri_total", "tri_kept", "tri_scored"))


# ---- 2: the input ends on, one past, and one past the second chunk of 64 ---------------------------------------------------
@pytest.mark.parametrize("n", [64, 65, 129])
def test_chunk_edges(pkg, O, reg, n):
    kw, src, tgt = polish_ref.edge_scene(pkg, n)
    _frame(reg, pkg, src, tgt, kw)
    _assert_polish(reg.polish(candidates=8, max_iter=16), _ref(O, f"edge{n}", src, tgt, kw, 8, 16), 8, f"n={n}")


def test_the_lane_deal_wraps(pkg, O, reg):
    """n = 9409: 148 chunks, the last of one element.  The refit deals its sums one lane per (chunk, component) over the 1024 threads of
    the workgroup, and 7 x 148 = 1036 and 9 x 148 = 1332 both exceed them: the deal's second round runs in both passes (at C1, the
    largest scene of the other cases, it never does).  C2's extent and tau with an inlier ratio of 0.03 (282 true correspondences,
    spread over all the chunks) and 300 hypotheses: the reference takes under a second."""
    cfg = pkg.synth.CONFIGS["C2"]
    sc = pkg.synth.make_scene(9409, 0.03, cfg.L, cfg.tau, cfg.seed)
    kw = dict(cfg.params(), max_triangles=300)
    _frame(reg, pkg, sc.src, sc.tgt, kw)
    exp = _ref(O, "wrap9409", sc.src, sc.tgt, kw, 2, 16)
    got = reg.polish(candidates=2, max_iter=16)
    _assert_polish(got, exp, 2, "n=9409")
    assert got["n_cand"] == 2 and all(int(c["iters"]) >= 1 for c in got["cand"])  # refits that changed (R, t) went through the deal


# ---- 3: one candidate, one refit IS the refit of SC_FLAG_REFINE ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["C0", "C1"])
def test_one_refit_of_the_winner_equals_flag_refine(pkg, reg, name):
    kw, src, tgt = _config(pkg, name)
    refined = _frame(reg, pkg, src, tgt, kw, flags=SC_FLAG_REFINE)
    on_it = reg.polish(candidates=1, max_iter=1)  # (the frame's SC_FLAG_REFINE changes its outputs, not its hypotheses)
    plain = _frame(reg, pkg, src, tgt, kw)
    got = reg.polish(candidates=1, max_iter=1)
    assert _flat(got).tobytes() == _flat(refined).tobytes() == _flat(on_it).tobytes()
    assert _flat(got).tobytes() != _flat(plain).tobytes() and int(got["cand"][0]["iters"]) == 1
    assert int(got["cand"][0]["rank"]) == plain["stats"]["best_rank"] and int(got["cand"][0]["score0"]) == plain["stats"]["best_count"]


# ---- 4: the truncated score modes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_score_modes(pkg, O, reg, mode):
    kw, src, tgt = _config(pkg, "C1")
    f = _frame(reg, pkg, src, tgt, kw, score_mode=mode)
    got = reg.polish(candidates=8, max_iter=16)
    _assert_polish(got, _ref(O, "C1", src, tgt, kw, 8, 16, mode), 8, f"mode {mode}")
    assert got["stats"]["best_count"] > f["stats"]["best_count"]  # a score that weighs residuals rises (test_polish_abi.py)


# ---- 5: a tight tau: many refits inside the one launch, and a runner-up may win ---------------------------------------------
def test_half_tau(pkg, O, reg):
    kw, src, tgt = _config(pkg, "C1")
    kw = dict(kw, tau=kw["tau"] / 2)
    _frame(reg, pkg, src, tgt, kw)
    exp = _ref(O, "C1", src, tgt, kw, 8, 16)
    assert max(c["iters"] for c in exp["cand"]) >= 9
    got = reg.polish(candidates=8, max_iter=16)
    _assert_polish(got, exp, 8, "tau / 2")
    cut = reg.polish(candidates=8, max_iter=4)  # ... and a limit that bites
    _assert_polish(cut, _ref(O, "C1", src, tgt, kw, 8, 4), 8, "tau / 2, max_iter 4")
    assert max(int(c["iters"]) for c in cut["cand"]) == 4


# ---- 6: fewer candidates than asked for; refits that are declined ----------------------------------------------------------
def test_fewer_candidates_than_asked_for_and_declined_refits(pkg, O, reg):
    kw, src, tgt = polish_ref.sparse_scene(pkg)
    _frame(reg, pkg, src, tgt, kw)
    exp = _ref(O, "sparse", src, tgt, kw, 64, 16)
    got = reg.polish(candidates=64, max_iter=16)
    _assert_polish(got, exp, 64, "sparse")
    assert 0 < got["n_cand"] < 64
    declined = [i for i, c in enumerate(exp["cand"]) if c["stop"] == "declined"]
    hyp = _hyp(O, "sparse", src, tgt, kw)
    assert declined and all(int(got["cand"][i]["iters"]) == 0 and nan_equal_bits(got["cand"][i]["Rt"], hyp["Rt"][exp["cand"][i]["rank"]])
                            for i in declined)


# ---- 7: independence --------------------------------------------------------------------------------------------------------
def _peel_flat(res):
    return (res["status"], _flat(res).tobytes(), res["mask"].tobytes(), res["stats"]["best_rank"], res["stats"]["best_count"])


@pytest.mark.parametrize("mode", [0, 1])
def test_polish_and_rounds_do_not_see_each_other(pkg, reg, mode):
    cfg = pkg.synth.CONFIGS["C1"]
    sc = pkg.synth.make_scene_motions(cfg.n, [0.6 * cfg.rho, 0.4 * cfg.rho], cfg.L, cfg.tau, cfg.seed)
    kw = cfg.params()
    _frame(reg, pkg, sc.src, sc.tgt, kw, score_mode=mode)
    alone = reg.polish(candidates=8, max_iter=16)
    again = reg.polish(candidates=8, max_iter=16)  # polish twice
    _same_polish(alone, again, "twice")
    rounds_after = [_peel_flat(reg.peel()) for _ in range(2)]
    between = reg.polish(candidates=8, max_iter=16)  # ... and after two rounds
    _same_polish(alone, between, "after two rounds")
    _frame(reg, pkg, sc.src, sc.tgt, kw, score_mode=mode)
    rounds_alone = [_peel_flat(reg.peel()) for _ in range(2)]
    assert rounds_after == rounds_alone
    _frame(reg, pkg, sc.src, sc.tgt, kw, score_mode=mode)
    first = _peel_flat(reg.peel())
    after_one = reg.polish(candidates=8, max_iter=16)  # one round, then polish
    _same_polish(alone, after_one, "after one round")
    assert first == rounds_alone[0] and _peel_flat(reg.peel()) == rounds_alone[1]


def _device_polish(pkg, r, q, n, k):
    import torch
    dev = torch.device("cuda:0")
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev)
    d_mask = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_cand = torch.full((k * 16,), 0x55, dtype=torch.int32, device=dev)
    d_n = torch.full((1,), 99, dtype=torch.int32, device=dev)
    rc, st = r.polish_device(q, d_Rt.data_ptr(), d_mask.data_ptr(), d_cand.data_ptr(), d_n.data_ptr())
    torch.cuda.synchronize()
    Rt = d_Rt.cpu().numpy()
    cand = np.frombuffer(d_cand.cpu().numpy().tobytes(), dtype=pkg.api.POLISH_CAND_DTYPE)
    return dict(status=rc, R=Rt[:9].reshape(3, 3), t=Rt[9:], mask=d_mask.cpu().numpy(), n_cand=int(d_n.cpu()[0]), cand=cand, stats=st)


def test_device_form_and_how_the_frame_was_enqueued(pkg, O):
    """The device form on a caller stream equals the host form, and the polish of a frame that was waited for, enqueued host-free
    (the second call of a repeated shape) or through sc_register_device_async + sc_wait is one and the same."""
    import torch
    kw, src, tgt = _config(pkg, "C1")
    n = src.shape[0]
    exp = _ref(O, "C1", src, tgt, kw, 8, 16)
    dev = torch.device("cuda:0")
    ds, dt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev)
    d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    p, q = pkg.make_params(**kw), pkg.make_polish_params(8, 16)
    r = pkg.Registrar(0)
    try:
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        results = []
        for how in ("waited", "host-free", "async"):
            if how == "async":
                r.register_device_async(ds.data_ptr(), dt.data_ptr(), n, p, d_Rt.data_ptr(), d_mask.data_ptr())
                rc, _ = r.wait()
            else:
                rc, _ = r.register_device(ds.data_ptr(), dt.data_ptr(), n, p, d_Rt.data_ptr(), d_mask.data_ptr())
            assert rc == SC_OK
            fast = r.debug_last()["fast_path"]
            print(how, "fast_path", fast)
            assert (fast == 0) == (how == "waited")
            got = _device_polish(pkg, r, q, n, 8)
            _assert_polish(got, exp, 8, how)
            results.append(got)
            host = r.polish(q)  # the host form on the same frame
            _same_polish(got, host, how + ": device form vs host form")
        # NULL d_cand / d_ncand are allowed
        rc, st = r.polish_device(q, d_Rt.data_ptr(), d_mask.data_ptr())
        torch.cuda.synchronize()
        assert rc == SC_OK and st["best_count"] == exp["best_count"] and nan_equal_bits(d_Rt.cpu().numpy(), exp["Rt"])
        assert np.array_equal(d_mask.cpu().numpy(), exp["mask"])
    finally:
        r.close()


# ---- 8: errors ------------------------------------------------------------------------------------------------------------------
def test_errors(pkg):
    L = pkg.load_library()
    kw, src, tgt = _config(pkg, "C0")
    r = pkg.Registrar(0)
    try:
        def status(**k):
            with pytest.raises(pkg.SacCotError) as e:
                r.polish(**k)
            return e.value.status, str(e.value)
        rc, text = status()  # no frame yet
        assert rc == SC_EINVAL and "no frame" in text
        assert b"no frame" in L.sc_last_error(r._h)
        _frame(r, pkg, src, tgt, kw)
        for bad in (dict(candidates=0), dict(candidates=65), dict(max_iter=0), dict(max_iter=65), dict(flags=1)):
            rc, text = status(**bad)
            assert rc == SC_EINVAL and "sc_polish" in text, bad
        q = pkg.make_polish_params()
        q.size = 28
        assert status(pparams=q)[0] == SC_EINVAL
        q = pkg.make_polish_params()
        q.reserved[2] = 1
        assert status(pparams=q)[0] == SC_EINVAL
        # NULL outputs on a real context
        st = pkg.ScStats(C.sizeof(pkg.ScStats))
        q = pkg.make_polish_params()
        assert L.sc_polish(r._h, C.byref(q), None, None, None, None, None, C.byref(st)) == SC_EINVAL
        assert L.sc_polish_device(r._h, C.byref(q), None, None, None, None, C.byref(st)) == SC_EINVAL
        assert r.polish()["status"] == SC_OK  # the refused calls left the frame alone
        # sc_match ends the frame
        rng = np.random.default_rng(3)
        r.match(rng.standard_normal((8, 4)).astype(np.float32), rng.standard_normal((9, 4)).astype(np.float32))
        assert status()[0] == SC_EINVAL
        # a frame call that returned SC_ENOHYP leaves no frame: three collinear, equidistant correspondences form a compatible
        # triangle that defines no rotation
        line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
        f = r.register(line, line, params=pkg.make_params(sigma=0.1, t_cmp=0.9, tau=0.1, min_len=0.1, max_triangles=10))
        assert f["status"] == SC_ENOHYP
        rc, text = status()
        assert rc == SC_EINVAL and "no frame" in text
        # an outstanding call
        import torch
        dev = torch.device("cuda:0")
        ds, dt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
        d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(len(src), dtype=torch.uint8, device=dev)
        r.register_device_async(ds.data_ptr(), dt.data_ptr(), len(src), pkg.make_params(**kw), d_Rt.data_ptr(), d_mask.data_ptr())
        rc, text = status()
        assert rc == SC_EINVAL and "outstanding" in text
        assert r.wait()[0] == SC_OK
        assert r.polish()["status"] == SC_OK
    finally:
        r.close()


# ---- 9: a context that never polishes holds what it held before ---------------------------------------------------------------
def test_workspace_is_allocated_by_the_first_polish_only(pkg):
    import torch
    kw, src, tgt = _config(pkg, "C0")
    n = len(src)
    dev = torch.device("cuda:0")
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    r = pkg.Registrar(0)
    try:
        # workspace_bytes is read through frames that have settled (a frame sizes its buffers by its history; with the host-free
        # enqueue off the same input takes the same path every time), so whatever moves afterwards is the polish's
        r.set_debug(no_fast=1)
        p = pkg.make_params(**kw)
        held = [r.register(src, tgt, params=p)["stats"]["workspace_bytes"] for _ in range(4)]
        assert held[2] == held[3] > 0, held
        held = held[1:]
        q = pkg.make_polish_params(8, 16)
        rc, st = r.polish_device(q, d_Rt.data_ptr(), d_mask.data_ptr())
        # the candidate list and 8 x ceil(500 / 64) x 16 doubles of chunk sums: two allocations of the workspace's smallest size
        assert rc == SC_OK and st["workspace_bytes"] == held[2] + 2 * 65536
        rc, st2 = r.polish_device(q, d_Rt.data_ptr(), d_mask.data_ptr())
        assert st2["workspace_bytes"] == st["workspace_bytes"]
        assert r.register(src, tgt, params=p)["stats"]["workspace_bytes"] == st["workspace_bytes"]
        # held against the cap of the frame's parameters
        r2 = pkg.Registrar(0)
        try:
            r2.set_debug(no_fast=1)
            for _ in range(4):
                f = r2.register(src, tgt, params=p)
            capped = pkg.make_params(**kw, max_workspace=f["stats"]["workspace_bytes"] + 4096)
            assert r2.register(src, tgt, params=capped)["status"] == SC_OK
            with pytest.raises(pkg.SacCotError) as e:
                r2.polish_device(q, d_Rt.data_ptr(), d_mask.data_ptr())
            assert e.value.status == -2
        finally:
            r2.close()
    finally:
        r.close()


# ---- 10: the frame's scores are the same whichever stage C2 kernel produced them ----------------------------------------------
@pytest.mark.parametrize("score_filter", [1, 2, 3])  # sc_debug.score_filter: 1 the plain fp32 kernel, 2 the linear filter, 3 the Gram filter
def test_frames_scored_by_every_c2_kernel(pkg, O, score_filter):
    kw, src, tgt = _config(pkg, "C1")
    r = pkg.Registrar(0)
    try:
        r.set_debug(score_filter=score_filter)
        _frame(r, pkg, src, tgt, kw)
        print("c2_kernel", r.debug_last()["c2_kernel"])
        _assert_polish(r.polish(candidates=8, max_iter=16), _ref(O, "C1", src, tgt, kw, 8, 16), 8, f"score_filter={score_filter}")
    finally:
        r.close()
