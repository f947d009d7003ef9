"""GPU: iterated fp64 refits for a batch's winners (include/saccot.h, sc_polish_batch / _device / _slots_device).

The expected value of every case is tests/polish_batch_ref.py — per problem polish_ref.iterate on the input record's Rt, then the CPU
restatement's score and mask — and everything is compared bit for bit: every field of every record, the Rt through nan_equal_bits,
every mask byte.  No tolerances.  The scenes are checked on the CPU by tests/test_polish_batch_abi.py (at most batch_ref.TRI_CAP
triangles a problem, so no workgroup of the registration runs long).
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref
import match_batch_ref as M
import polish_batch_ref as PB
from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
SC_FLAG_EXACT_TOTAL, SC_FLAG_REFINE = 2, 8

_CACHE = {}


def _pack(problems):
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.uint32)
    return np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems]), off


def _layout(pkg, src, tgt, soa):
    return (np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)) if soa else (src, tgt)


def _register(reg, pkg, problems, kw, mode=0, soa=False):
    """sc_register_batch on the packed batch -> (records, mask, packed src, tgt, offset, params)"""
    src, tgt, off = _pack(problems)
    src, tgt = _layout(pkg, src, tgt, soa)
    p = pkg.make_params(**kw, score_mode=mode, layout=pkg.SC_SOA if soa else pkg.SC_AOS)
    recs, mask = reg.register_batch_raw(src, tgt, off, p)
    return recs, mask, src, tgt, off, p


def _both(reg, pkg, problems, kw, mode, max_iter, soa=False, recs=None):
    """sc_register_batch then sc_polish_batch -> (batch records, polish records, polish mask, offset)"""
    r, _, src, tgt, off, p = _register(reg, pkg, problems, kw, mode, soa)
    if recs is not None:
        r = recs
    pol, pmask = reg.polish_batch_raw(src, tgt, off, p, pkg.make_polish_params(candidates=1, max_iter=max_iter), r)
    return r, pol, pmask, off


def _mixed_ref(pkg, O, tau, mode, max_iter):
    """the reference of the mixed batch, once per session and parameter set; never modified"""
    key = (tau, mode, max_iter)
    if key not in _CACHE:
        problems = PB.mixed(pkg)
        if ("recs", tau, mode) not in _CACHE:
            _CACHE[("recs", tau, mode)] = batch_ref.batch(O, problems, PB.kw_of(tau), mode)
        _CACHE[key] = PB.batch(O, problems, _CACHE[("recs", tau, mode)][0], tau, mode, max_iter)
    return _CACHE[("recs", tau, mode)], _CACHE[key]


def _assert_polish(pol, pmask, off, exp, what=""):
    erecs, emasks = exp
    assert len(pol) == len(erecs), what
    for b in range(len(pol)):
        g, e = pol[b], erecs[b]
        print(what, b, [int(g[f]) for f in PB.FIELDS], "| expected", [int(e[f]) for f in PB.FIELDS])
        assert [int(g[f]) for f in PB.FIELDS] == [int(e[f]) for f in PB.FIELDS], (what, b)
        assert nan_equal_bits(g["Rt"], e["Rt"]), (what, b)
        assert np.array_equal(pmask[off[b]: off[b + 1]], emasks[b]), (what, b)


# ---- 1: the mixed batch: both layouts, every max_iter, both scales, all three score modes ------------------------------------------
CASES = [(tau, 0, mi) for tau in PB.TAUS for mi in PB.MAX_ITERS] + [(0.02, mode, mi) for mode in (1, 2) for mi in PB.MAX_ITERS]


@pytest.mark.parametrize("tau,mode,max_iter", CASES)
def test_mixed_batch_equals_the_reference(pkg, O, reg, tau, mode, max_iter):
    problems = PB.mixed(pkg)
    (erecs, _), exp = _mixed_ref(pkg, O, tau, mode, max_iter)
    for soa in (False, True):
        recs, pol, pmask, off = _both(reg, pkg, problems, PB.kw_of(tau), mode, max_iter, soa)
        assert list(recs["status"]) == list(erecs["status"]) and all(nan_equal_bits(a["Rt"], b["Rt"]) for a, b in zip(recs, erecs))
        _assert_polish(pol, pmask, off, exp, f"tau={tau} mode={mode} max_iter={max_iter} soa={soa}")
        ok = recs["status"] == SC_OK
        assert ok.sum() >= 9 and np.array_equal(pol["score0"][ok], recs["best_count"][ok])  # score0 == best_count of the batch record
    if max_iter == 16 and mode == 0 and tau == 0.02:  # the list form returns the same, problem by problem
        out = reg.register_batch_polished(problems, params=pkg.make_params(**PB.kw_of(tau)), max_iter=16)
        for b, o in enumerate(out):
            q = o["polished"]
            assert (o["status"], o["stats"]["best_count"]) == (int(recs[b]["status"]), int(recs[b]["best_count"]))
            assert [q["status"], q["score0"], q["score"], q["iters"], q["stop"]] == [int(pol[b][f]) for f in PB.FIELDS]
            assert np.concatenate([q["R"].ravel(), q["t"]]).tobytes() == pol[b]["Rt"].tobytes()
            assert np.array_equal(q["mask"], pmask[off[b]: off[b + 1]])


# ---- 2: against the single-problem path: sc_register then sc_polish(candidates = 1) -------------------------------------------------
@pytest.mark.parametrize("mode,max_iter", [(0, 16), (0, 2), (1, 16)])
def test_equals_sc_register_then_sc_polish(pkg, O, reg, mode, max_iter):
    problems = PB.mixed(pkg)
    kw = PB.kw_of(0.02)
    recs, pol, pmask, off = _both(reg, pkg, problems, kw, mode, max_iter)
    polished = 0
    for b, (s, t) in enumerate(problems):
        solo = reg.register(s, t, params=pkg.make_params(**kw, score_mode=mode, flags=SC_FLAG_EXACT_TOTAL))
        assert solo["status"] == int(recs[b]["status"]), b
        if solo["status"] != SC_OK:  # no frame, no polish: the status is passed through
            assert int(pol[b]["status"]) == solo["status"] and pol[b]["Rt"].tobytes() == batch_ref.IDENT.tobytes()
            continue
        one = reg.polish(candidates=1, max_iter=max_iter)
        k = one["cand"][0]
        assert one["status"] == SC_OK and one["n_cand"] == 1, b
        assert nan_equal_bits(pol[b]["Rt"], np.concatenate([one["R"].ravel(), one["t"]])) and nan_equal_bits(pol[b]["Rt"], k["Rt"]), b
        assert np.array_equal(pmask[off[b]: off[b + 1]], one["mask"]), b
        assert (int(pol[b]["score0"]), int(pol[b]["score"]), int(pol[b]["iters"])) == (int(k["score0"]), int(k["score"]), int(k["iters"])), b
        polished += 1
    assert polished >= 9


# ---- 3: one refit is SC_FLAG_REFINE's -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", PB.TAUS)
def test_one_refit_equals_sc_register_with_refine(pkg, O, reg, tau):
    problems = PB.mixed(pkg)
    kw = PB.kw_of(tau)
    recs, pol, _, _ = _both(reg, pkg, problems, kw, 0, 1)
    seen = 0
    for b, (s, t) in enumerate(problems):
        solo = reg.register(s, t, params=pkg.make_params(**kw, flags=SC_FLAG_EXACT_TOTAL | SC_FLAG_REFINE))
        if solo["status"] != SC_OK:
            assert int(pol[b]["status"]) == solo["status"]
            continue
        assert nan_equal_bits(pol[b]["Rt"], np.concatenate([solo["R"].ravel(), solo["t"]])), (tau, b)
        seen += 1
    assert seen >= 9


# ---- 4: a record is a function of its own problem, its input pose and the parameters ----------------------------------------------
def test_independence_of_position_neighbours_history_and_the_mask_buffer(pkg, O, reg):
    import torch
    problems = PB.mixed(pkg)
    kw = PB.kw_of(0.02)
    recs, pol, pmask, off = _both(reg, pkg, problems, kw, 0, 16)
    _assert_polish(pol, pmask, off, _mixed_ref(pkg, O, 0.02, 0, 16)[1], "base")
    base = [(pol[b].tobytes(), pmask[off[b]: off[b + 1]].tobytes()) for b in range(len(problems))]

    def check(order, what):
        _, q, m, o = _both(reg, pkg, [problems[b] for b in order], kw, 0, 16)
        for pos, b in enumerate(order):
            assert (q[pos].tobytes(), m[o[pos]: o[pos + 1]].tobytes()) == base[b], (what, b)

    nb = len(problems)
    check(list(range(nb))[::-1], "reversed")
    for b in range(nb):
        check([b], "alone")
    # the records need not come from this context's registration: the same bytes handed in by the caller, on a used context
    src, tgt, _ = _pack(problems)
    p = pkg.make_params(**kw)
    q = pkg.make_polish_params(candidates=1, max_iter=16)
    again, again_mask = reg.polish_batch_raw(src, tgt, off, p, q, recs.copy())
    assert again.tobytes() == pol.tobytes() and np.array_equal(again_mask, pmask)
    # the device form: two launches on a caller's stream, d_mask once the registration's own buffer, once a separate one
    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    outs = []
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    reg.set_stream(stream.cuda_stream)
    try:
        for alias in (True, False):
            d_res = torch.zeros(nb * 80, dtype=torch.uint8, device="cuda")
            d_pol = torch.full((nb * 64,), 0xAB, dtype=torch.uint8, device="cuda")
            d_mask = torch.full((int(off[-1]),), 7, dtype=torch.uint8, device="cuda")
            d_mask2 = d_mask if alias else torch.full((int(off[-1]),), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            reg.register_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_res.data_ptr(), d_mask.data_ptr())
            reg.polish_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, q, d_res.data_ptr(), d_pol.data_ptr(), d_mask2.data_ptr())
            stream.synchronize()
            outs.append((d_res.cpu().numpy().tobytes(), d_pol.cpu().numpy().tobytes(), d_mask2.cpu().numpy()))
    finally:
        reg.set_stream(None)
    for res_bytes, pol_bytes, m in outs:
        assert res_bytes == recs.tobytes()  # d_res is read, never written
        assert pol_bytes == pol.tobytes() and np.array_equal(m, pmask)


# ---- 5: bad and empty problems between good ones ------------------------------------------------------------------------------------
def test_bad_and_empty_problems_between_good_ones(pkg, O, reg):
    kw = PB.kw_of(0.02)
    g128, g64, g65, g129, e3 = (batch_ref.scene(pkg, n, rho) for n, rho in ((128, .3), (64, .3), (65, .3), (129, .3), (3, 1.0)))
    clean = [g128, g64, e3, g129, g65]
    recs, _, _, _, off, p = _register(reg, pkg, clean, kw)
    assert list(recs["status"]) == [SC_OK, SC_OK, SC_ENOHYP, SC_OK, SC_OK]
    nan_t = g64[1].copy(); nan_t[17, 2] = np.nan
    problems = [g128, (g64[0], nan_t), e3, g129, g65]  # [1]: a NaN coordinate under an SC_OK record; [2]: SC_ENOHYP
    hand = recs.copy()
    hand["Rt"][3][5] = np.nan                          # [3]: a hand-made record with SC_OK and a NaN in Rt
    src, tgt, _ = _pack(problems)
    q = pkg.make_polish_params(candidates=1, max_iter=16)
    for soa in (False, True):
        a, b = _layout(pkg, src, tgt, soa)
        pl = pkg.make_params(**kw, layout=pkg.SC_SOA if soa else pkg.SC_AOS)
        pol, pmask = reg.polish_batch_raw(a, b, off, pl, q, hand)
        _assert_polish(pol, pmask, off, PB.batch(O, problems, hand, 0.02, 0, 16), f"soa={soa}")
        assert list(pol["status"]) == [SC_OK, SC_EINVAL, SC_ENOHYP, SC_EINVAL, SC_OK]
        for k in (1, 2, 3):  # the output shape of a problem without a pose
            assert pol[k]["Rt"].tobytes() == batch_ref.IDENT.tobytes() and not pmask[off[k]: off[k + 1]].any()
            assert [int(pol[k][f]) for f in PB.FIELDS[1:]] == [0, 0, 0, PB.STOP_DECLINED]
    # the registration's own SC_EINVAL (it found the NaN itself) is passed through as well
    r2, pol2, pmask2, off2 = _both(reg, pkg, problems, kw, 0, 16)
    assert list(r2["status"]) == [SC_OK, SC_EINVAL, SC_ENOHYP, SC_OK, SC_OK] and list(pol2["status"]) == list(r2["status"])
    # the neighbours are bit-identical to a batch without the bad ones
    _, few, few_mask, few_off = _both(reg, pkg, [g128, g65], kw, 0, 16)
    for pos, k in enumerate((0, 4)):
        assert few[pos].tobytes() == pol[k].tobytes() == pol2[k].tobytes()
        assert np.array_equal(few_mask[few_off[pos]: few_off[pos + 1]], pmask[off[k]: off[k + 1]])
        assert np.array_equal(few_mask[few_off[pos]: few_off[pos + 1]], pmask2[off2[k]: off2[k + 1]])


# ---- 6: a winner whose first refit is declined --------------------------------------------------------------------------------------
def test_the_sparse_problem_keeps_its_input_pose(pkg, O, reg):
    kw, src, tgt = PB.sparse(pkg)
    g64 = batch_ref.scene(pkg, 64, .3)
    problems = [g64, (src, tgt), g64]
    recs, pol, pmask, off = _both(reg, pkg, problems, kw, 0, 16)
    erecs, _ = batch_ref.batch(O, problems, kw)
    assert all(nan_equal_bits(a["Rt"], b["Rt"]) for a, b in zip(recs, erecs)) and list(recs["status"]) == list(erecs["status"])
    _assert_polish(pol, pmask, off, PB.batch(O, problems, erecs, kw["tau"], 0, 16), "sparse")
    assert (int(pol[1]["status"]), int(pol[1]["iters"]), int(pol[1]["stop"])) == (SC_OK, 0, PB.STOP_DECLINED)
    assert pol[1]["Rt"].tobytes() == recs[1]["Rt"].tobytes() and 0 < pol[1]["score"] == pol[1]["score0"] == recs[1]["best_count"] < 3


# ---- 7: the slot form behind sc_register_batch_features_device ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mutual", "knn2"])
def test_slot_form_equals_the_plain_form_on_the_gathered_correspondences(pkg, O, reg, mode):
    import torch
    knn = 1 if mode == "mutual" else 2
    scenes = [M.feature_scene(n, rho, noise, 4100 + n) for n, rho, noise in ((40, .6, .001), (1, 1.0, 0.0), (100, .4, .001), (64, .5, .001), (200, .3, .001))]
    problems = [list(s[:4]) for s in scenes]
    problems[3][1] = problems[3][1].copy(); problems[3][1][5, 0] = np.inf  # a non-finite descriptor: the match flags this problem
    mp = pkg.api.make_match_params(33, knn=knn, mutual=(mode == "mutual"))
    so = reg._offsets([len(s[1]) for s in problems]); to = reg._offsets([len(s[3]) for s in problems])
    fsrc, ftgt = np.concatenate([s[1] for s in problems]), np.concatenate([s[3] for s in problems])
    nb, slots = len(problems), int(so[-1]) * knn
    q = pkg.make_polish_params(candidates=1, max_iter=16)
    kw = dict(M.KW, tau=0.02)
    seen = None
    for soa in (False, True):
        p = pkg.make_params(**kw, layout=pkg.SC_SOA if soa else pkg.SC_AOS)
        src, tgt = _layout(pkg, np.concatenate([s[0] for s in problems]), np.concatenate([s[2] for s in problems]), soa)
        dev = {k: torch.from_numpy(v).cuda() for k, v in dict(src=src, fsrc=fsrc, tgt=tgt, ftgt=ftgt).items()}
        d_res = torch.zeros(nb * 80, dtype=torch.uint8, device="cuda"); d_pol = torch.full((nb * 64,), 0xAB, dtype=torch.uint8, device="cuda")
        d_corr = torch.full((slots, 2), -7, dtype=torch.int32, device="cuda"); d_d2 = torch.zeros(slots, dtype=torch.float32, device="cuda")
        d_count = torch.full((nb, 2), 9, dtype=torch.int32, device="cuda")
        d_mask = torch.full((slots,), 7, dtype=torch.uint8, device="cuda"); d_pmask = torch.full((slots,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        reg.register_batch_features_device(dev["src"].data_ptr(), dev["fsrc"].data_ptr(), so, dev["tgt"].data_ptr(), dev["ftgt"].data_ptr(), to,
                                           mp, p, d_res.data_ptr(), d_corr.data_ptr(), d_d2.data_ptr(), d_count.data_ptr(), d_mask.data_ptr())
        reg.polish_batch_slots_device(dev["src"].data_ptr(), so, dev["tgt"].data_ptr(), to, knn, p, q, d_corr.data_ptr(), d_count.data_ptr(),
                                      d_res.data_ptr(), d_pol.data_ptr(), d_pmask.data_ptr())
        torch.cuda.synchronize()
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE)
        pol = np.frombuffer(d_pol.cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE)
        corr, count, pmask = d_corr.cpu().numpy(), d_count.cpu().numpy().astype(np.uint32), d_pmask.cpu().numpy()
        print(mode, soa, list(res["status"]), count.tolist(), [tuple(int(o[f]) for f in PB.FIELDS) for o in pol])
        assert list(res["status"]) == [SC_OK, SC_ENOHYP, SC_OK, SC_EINVAL, SC_OK] and count[1, 0] < 3 and count[3].tolist() == [0, 1]
        # the flagged and the short problem pass their input status through
        for b in (1, 3):
            assert int(pol[b]["status"]) == int(res[b]["status"]) and pol[b]["Rt"].tobytes() == batch_ref.IDENT.tobytes()
            assert [int(pol[b][f]) for f in PB.FIELDS[1:]] == [0, 0, 0, PB.STOP_DECLINED]
            lo = int(so[b]) * knn
            assert not pmask[lo: lo + int(count[b, 0])].any()
        # the others: sc_polish_batch on the gathered correspondences, packed here from corr / count
        good = [0, 2, 4]
        packed = []
        for b in good:
            lo, n = int(so[b]) * knn, int(count[b, 0])
            packed.append((np.ascontiguousarray(problems[b][0][corr[lo: lo + n, 0]]), np.ascontiguousarray(problems[b][2][corr[lo: lo + n, 1]])))
        gs, gt, goff = _pack(packed)
        plain, plain_mask = reg.polish_batch_raw(gs, gt, goff, pkg.make_params(**kw), q, res[good])
        for pos, b in enumerate(good):
            lo, n = int(so[b]) * knn, int(count[b, 0])
            assert n == goff[pos + 1] - goff[pos] and pol[b].tobytes() == plain[pos].tobytes(), (mode, soa, b)
            assert np.array_equal(pmask[lo: lo + n], plain_mask[goff[pos]: goff[pos + 1]]), (mode, soa, b)
        _assert_polish(plain, plain_mask, goff, PB.batch(O, packed, res[good], 0.02, 0, 16), f"slots {mode} soa={soa}")
        assert int(plain["iters"].max()) >= 1
        if seen is None:
            seen = (pol.tobytes(), pmask.tobytes(), count.tobytes())
        else:  # the layout of the points does not matter
            assert pol.tobytes() == seen[0] and count.tobytes() == seen[2]


# ---- 8: what is refused, and what a call leaves --------------------------------------------------------------------------------------
def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def test_refusals_leave_the_context_usable(pkg, O, reg):
    import torch
    L = reg._lib
    kw = PB.kw_of(0.02)
    s, t = batch_ref.scene(pkg, 128, .3)
    recs, _, _, _, off, p = _register(reg, pkg, [(s, t)], kw)
    good_q = pkg.make_polish_params(candidates=1, max_iter=16)
    good, good_mask = reg.polish_batch_raw(s, t, off, p, good_q, recs)
    assert good[0]["status"] == SC_OK
    u32 = lambda *a: np.array(a, np.uint32)  # noqa: E731
    big = np.zeros((513, 3), np.float32)
    res_big = np.zeros(3, pkg.BATCH_RESULT_DTYPE)

    def host(src, tgt, o, nb, pp, qq, res=recs):
        pol = np.zeros(max(nb, 1), PB.RESULT_DTYPE); mask = np.zeros(max(int(o[-1]), 1), np.uint8)
        rc = L.sc_polish_batch(reg._h, _ptr(src, C.c_float), _ptr(tgt, C.c_float), _ptr(o, C.c_uint32), nb, C.byref(pp) if pp else None,
                               C.byref(qq) if qq else None, None if res is None else res.ctypes.data_as(C.c_void_p),
                               pol.ctypes.data_as(C.c_void_p), _ptr(mask, C.c_uint8))
        return rc, L.sc_last_error(reg._h).decode()

    rsv = pkg.make_polish_params(candidates=1); rsv.reserved[2] = 1
    cases = {
        "a NULL src": lambda: host(None, t, off, 1, p, good_q),
        "NULL records": lambda: host(s, t, off, 1, p, good_q, None),
        "NULL polish params": lambda: host(s, t, off, 1, p, None),
        "candidates = 8": lambda: host(s, t, off, 1, p, pkg.make_polish_params(candidates=8)),
        "candidates = 0": lambda: host(s, t, off, 1, p, pkg.make_polish_params(candidates=0)),
        "max_iter = 0": lambda: host(s, t, off, 1, p, pkg.make_polish_params(candidates=1, max_iter=0)),
        "max_iter = 65": lambda: host(s, t, off, 1, p, pkg.make_polish_params(candidates=1, max_iter=65)),
        "a flag": lambda: host(s, t, off, 1, p, pkg.make_polish_params(candidates=1, flags=1)),
        "a reserved word": lambda: host(s, t, off, 1, p, rsv),
        "n_b = 2": lambda: host(s, t, u32(0, 2), 1, p, good_q),
        "n_b = 513": lambda: host(big, big, u32(0, 513), 1, p, good_q),
        "n_problems = 0": lambda: host(s, t, u32(0), 0, p, good_q),
        "a decreasing offset": lambda: host(s, t, u32(0, 64, 60, 128), 3, p, good_q, res_big),
        "SC_FLAG_REFINE": lambda: host(s, t, off, 1, pkg.make_params(**kw, flags=SC_FLAG_REFINE), good_q),
        "shard_world = 2": lambda: host(s, t, off, 1, pkg.make_params(**kw, shard_world=2), good_q),
    }
    for what, call in cases.items():
        rc, err = call()
        print(what, rc, err)
        assert rc == SC_EINVAL and "sc_polish_batch" in err, what
        again, again_mask = reg.polish_batch_raw(s, t, off, p, good_q, recs)  # the context stays usable
        assert again.tobytes() == good.tobytes() and np.array_equal(again_mask, good_mask), what
    # the device forms: refused on the host, so the outputs keep what they held
    d_s, d_t = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
    d_res = torch.from_numpy(np.frombuffer(recs.tobytes(), np.uint8).copy()).cuda()
    d_pol = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda"); d_mask = torch.full((128,), 7, dtype=torch.uint8, device="cuda")
    d_corr = torch.zeros((512, 2), dtype=torch.int32, device="cuda"); d_count = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev_cases = {
        "device: candidates = 2": lambda: reg.polish_batch_device(d_s.data_ptr(), d_t.data_ptr(), off, p, pkg.make_polish_params(candidates=2),
                                                                  d_res.data_ptr(), d_pol.data_ptr(), d_mask.data_ptr()),
        "device: a NULL output": lambda: reg.polish_batch_device(d_s.data_ptr(), d_t.data_ptr(), off, p, good_q, d_res.data_ptr(), 0, d_mask.data_ptr()),
        "slots: knn = 0": lambda: reg.polish_batch_slots_device(d_s.data_ptr(), off, d_t.data_ptr(), off, 0, p, good_q, d_corr.data_ptr(),
                                                                d_count.data_ptr(), d_res.data_ptr(), d_pol.data_ptr(), d_mask.data_ptr()),
        "slots: knn = 5": lambda: reg.polish_batch_slots_device(d_s.data_ptr(), off, d_t.data_ptr(), off, 5, p, good_q, d_corr.data_ptr(),
                                                                d_count.data_ptr(), d_res.data_ptr(), d_pol.data_ptr(), d_mask.data_ptr()),
        "slots: ns * knn > SC_BATCH_MAX_N": lambda: reg.polish_batch_slots_device(d_s.data_ptr(), u32(0, 300), d_t.data_ptr(), u32(0, 128), 2, p, good_q,
                                                                                  d_corr.data_ptr(), d_count.data_ptr(), d_res.data_ptr(),
                                                                                  d_pol.data_ptr(), d_mask.data_ptr()),
        "slots: candidates = 8": lambda: reg.polish_batch_slots_device(d_s.data_ptr(), off, d_t.data_ptr(), off, 1, p, pkg.make_polish_params(),
                                                                       d_corr.data_ptr(), d_count.data_ptr(), d_res.data_ptr(), d_pol.data_ptr(),
                                                                       d_mask.data_ptr()),
    }
    for what, call in dev_cases.items():
        with pytest.raises(pkg.SacCotError) as e:
            call()
        print(what, e.value)
        assert e.value.status == SC_EINVAL and "sc_polish_batch" in str(e.value), what
    torch.cuda.synchronize()
    assert (d_pol.cpu().numpy() == 0xAB).all() and (d_mask.cpu().numpy() == 7).all()  # nothing was enqueued
    reg.polish_batch_device(d_s.data_ptr(), d_t.data_ptr(), off, p, good_q, d_res.data_ptr(), d_pol.data_ptr(), d_mask.data_ptr())
    torch.cuda.synchronize()
    assert d_pol.cpu().numpy().tobytes() == good.tobytes() and np.array_equal(d_mask.cpu().numpy(), good_mask)
    # a call outstanding on the context
    d_rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_m = torch.zeros(128, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reg.register_device_async(d_s.data_ptr(), d_t.data_ptr(), 128, p, d_rt.data_ptr(), d_m.data_ptr())
    rc, err = host(s, t, off, 1, p, good_q)
    assert rc == SC_EINVAL and "outstanding" in err
    rc, _ = reg.wait()
    assert rc == SC_OK
    # a polish-batch call ends the frame and leaves none
    assert reg.register(s, t, params=p)["status"] == SC_OK
    reg.polish_batch_raw(s, t, off, p, good_q, recs)
    for call in (reg.peel, reg.polish):
        with pytest.raises(pkg.SacCotError) as e:
            call()
        assert e.value.status == SC_EINVAL


# ---- 9: a context that never calls these entries allocates nothing new ----------------------------------------------------------------
def test_workspace_appears_with_the_first_call(pkg):
    r = pkg.Registrar(0)
    try:
        s, t = batch_ref.scene(pkg, 128, .3)
        p = pkg.make_params(**PB.kw_of(0.02))
        recs, _ = r.register_batch_raw(s, t, np.array([0, 128], np.uint32), p)
        first = r.register(s, t, params=p)["stats"]["workspace_bytes"]
        assert r.register(s, t, params=p)["stats"]["workspace_bytes"] == first
        r.polish_batch_raw(s, t, np.array([0, 128], np.uint32), p, pkg.make_polish_params(candidates=1), recs)
        second = r.register(s, t, params=p)["stats"]["workspace_bytes"]
        r.polish_batch_raw(s, t, np.array([0, 128], np.uint32), p, pkg.make_polish_params(candidates=1), recs)
        print(first, second)
        assert second > first and r.register(s, t, params=p)["stats"]["workspace_bytes"] == second
    finally:
        r.close()
