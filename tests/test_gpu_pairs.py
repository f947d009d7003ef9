"""GPU: listed pairs of shared keypoint sets (include/saccot.h, sc_match_pairs* / sc_register_pairs_features* /
sc_polish_pairs_slots_device).

Two comparators for every case, both bit for bit on the specified ranges (the first n_p entries of a slot, the count pairs, every
byte of every record): tests/pairs_ref.py — the composed CPU references per pair — and the PACKED entries of this library on the
pair list expanded into packed arrays in list order, which is what the contract promises to equal.  No tolerances.  The table and
the list are checked on the CPU by tests/test_pairs_abi.py (at most batch_ref.TRI_CAP triangles a pair, so no workgroup runs long).
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref
import pairs_ref as P
import polish_batch_ref as PB
from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
FIELDS = ("status", "n", "edges", "tri_kept", "tri_total", "best_rank", "best_count")
MUTUAL = dict(knn=1, mutual=True)
KW02 = dict(P.KW, tau=0.02)  # the polish tests': refits that move

_REF = {}


def _ref(key, make):
    """a reference, once per session; never modified"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _junk(torch, shape, dtype, value):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _outputs(torch, npairs, slots, features, polish):
    o = dict(corr=_junk(torch, (slots, 2), torch.int32, -7), d2=_junk(torch, (slots,), torch.float32, -1.0),
             count=_junk(torch, (npairs, 2), torch.int32, 9))
    if features:
        o.update(res=_junk(torch, (npairs * 80,), torch.uint8, 0xAB), mask=_junk(torch, (slots,), torch.uint8, 7))
    if polish:
        o.update(pol=_junk(torch, (npairs * 64,), torch.uint8, 0xAB), pmask=_junk(torch, (slots,), torch.uint8, 7))
    return o


def _to_host(pkg, o, slot):
    out = dict(slot=np.asarray(slot, np.int64), corr=o["corr"].cpu().numpy(), d2=o["d2"].cpu().numpy(),
               count=o["count"].cpu().numpy().astype(np.uint32))
    if "res" in o:
        out.update(res=np.frombuffer(o["res"].cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE), mask=o["mask"].cpu().numpy())
    if "pol" in o:
        out.update(pol=np.frombuffer(o["pol"].cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE), pmask=o["pmask"].cpu().numpy())
    return out


def _points(pkg, pts, p):
    return np.ascontiguousarray(pts.T) if p is not None and p.layout == pkg.SC_SOA else pts


def run_pairs(reg, pkg, tab, pairs, mp, p=None, q=None):
    """the device forms on the table and the list -> the outputs on the host (the match alone; with p the registration; with q the
    polish behind it)"""
    import torch
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    slot = reg.pairs_layout(tab["set_off"], pairs, int(mp.knn))
    d_feat = torch.from_numpy(tab["feat"]).cuda()
    o = _outputs(torch, len(pairs), int(slot[-1]), p is not None, q is not None)
    torch.cuda.synchronize()
    if p is None:
        reg.match_pairs_device(d_feat.data_ptr(), tab["set_off"], pairs, mp, o["corr"].data_ptr(), o["d2"].data_ptr(), o["count"].data_ptr())
    else:
        d_pts = torch.from_numpy(_points(pkg, tab["pts"], p)).cuda()
        reg.register_pairs_features_device(d_pts.data_ptr(), d_feat.data_ptr(), tab["set_off"], pairs, mp, p, o["res"].data_ptr(),
                                           o["corr"].data_ptr(), o["d2"].data_ptr(), o["count"].data_ptr(), o["mask"].data_ptr())
        if q is not None:
            reg.polish_pairs_slots_device(d_pts.data_ptr(), tab["set_off"], pairs, int(mp.knn), p, q, o["corr"].data_ptr(),
                                          o["count"].data_ptr(), o["res"].data_ptr(), o["pol"].data_ptr(), o["pmask"].data_ptr())
    torch.cuda.synchronize()
    return _to_host(pkg, o, slot)


def run_packed(reg, pkg, tab, pairs, mp, p=None, q=None):
    """the parent's way: the list expanded into packed arrays in list order (every set copied once per pair it takes part in), then
    the packed entries"""
    import torch
    problems = P.expand(tab, pairs)
    so = reg._offsets([len(s[1]) for s in problems]); to = reg._offsets([len(s[3]) for s in problems])
    slot = so.astype(np.int64) * int(mp.knn)
    d_fs = torch.from_numpy(np.concatenate([s[1] for s in problems])).cuda()
    d_ft = torch.from_numpy(np.concatenate([s[3] for s in problems])).cuda()
    o = _outputs(torch, len(problems), int(slot[-1]), p is not None, q is not None)
    torch.cuda.synchronize()
    if p is None:
        reg.match_batch_device(d_fs.data_ptr(), so, d_ft.data_ptr(), to, mp, o["corr"].data_ptr(), o["d2"].data_ptr(), o["count"].data_ptr())
    else:
        d_ps = torch.from_numpy(_points(pkg, np.concatenate([s[0] for s in problems]), p)).cuda()
        d_pt = torch.from_numpy(_points(pkg, np.concatenate([s[2] for s in problems]), p)).cuda()
        reg.register_batch_features_device(d_ps.data_ptr(), d_fs.data_ptr(), so, d_pt.data_ptr(), d_ft.data_ptr(), to, mp, p, o["res"].data_ptr(),
                                           o["corr"].data_ptr(), o["d2"].data_ptr(), o["count"].data_ptr(), o["mask"].data_ptr())
        if q is not None:
            reg.polish_batch_slots_device(d_ps.data_ptr(), so, d_pt.data_ptr(), to, int(mp.knn), p, q, o["corr"].data_ptr(), o["count"].data_ptr(),
                                          o["res"].data_ptr(), o["pol"].data_ptr(), o["pmask"].data_ptr())
    torch.cuda.synchronize()
    return _to_host(pkg, o, slot)


def pair_bytes(out, p):
    """everything the contract specifies of pair p, as bytes: the count pair, the first n_p entries of its slot, its records"""
    lo, n = int(out["slot"][p]), int(out["count"][p, 0])
    parts = [out["count"][p].tobytes(), out["corr"][lo: lo + n].tobytes(), out["d2"][lo: lo + n].tobytes()]
    if "res" in out:
        parts += [out["res"][p].tobytes(), out["mask"][lo: lo + n].tobytes()]
    if "pol" in out:
        parts += [out["pol"][p].tobytes(), out["pmask"][lo: lo + n].tobytes()]
    return tuple(parts)


def all_bytes(out):
    return [pair_bytes(out, p) for p in range(len(out["count"]))]


def assert_same(got, exp, what):
    assert np.array_equal(got["slot"], exp["slot"]), what  # the layout coincides with the packed form's
    for p, (g, e) in enumerate(zip(all_bytes(got), all_bytes(exp))):
        assert g == e, (what, p)


def assert_match_ref(out, ref, what):
    assert len(out["count"]) == len(ref)
    for p, (corr, d2, n, flag) in enumerate(ref):
        lo = int(out["slot"][p])
        assert out["count"][p].tolist() == [n, flag], (what, p, out["count"][p].tolist(), n, flag)
        assert np.array_equal(out["corr"][lo: lo + n], corr) and out["d2"][lo: lo + n].tobytes() == d2.tobytes(), (what, p)


def assert_features_ref(out, ref, what):
    assert_match_ref(out, [(r["corr"], r["d2"], r["n"], r["flag"]) for r in ref], what)
    for p, r in enumerate(ref):
        g, e, lo = out["res"][p], r["rec"], int(out["slot"][p])
        print(what, p, "n", r["n"], [int(g[f]) for f in FIELDS], "| expected", [int(e[f]) for f in FIELDS])
        assert [int(g[f]) for f in FIELDS] == [int(e[f]) for f in FIELDS], (what, p)
        assert nan_equal_bits(g["Rt"], e["Rt"]), (what, p)
        assert np.array_equal(out["mask"][lo: lo + len(r["mask"])], r["mask"]), (what, p)


def assert_polish_ref(out, ref, what):
    for p, (e, emask) in enumerate(ref):
        g, lo = out["pol"][p], int(out["slot"][p])
        assert [int(g[f]) for f in PB.FIELDS] == [int(e[f]) for f in PB.FIELDS], (what, p, [int(g[f]) for f in PB.FIELDS], [int(e[f]) for f in PB.FIELDS])
        assert nan_equal_bits(g["Rt"], e["Rt"]), (what, p)
        assert np.array_equal(out["pmask"][lo: lo + len(emask)], emask), (what, p)


# ---- 1: the match ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mutual_ratio", "knn2", "knn4"])
def test_match_pairs_equals_the_reference_and_the_packed_form(pkg, reg, mode):
    mkw = dict(mutual_ratio=dict(knn=1, mutual=True, ratio=0.8), knn2=dict(knn=2), knn4=dict(knn=4))[mode]
    tab = P.table()
    mp = pkg.api.make_match_params(P.DIM, **mkw)
    got = run_pairs(reg, pkg, tab, P.PAIRS, mp)
    print(mode, got["count"][:, 0].tolist())
    assert_match_ref(got, _ref(("match", mode), lambda: P.match(tab, P.PAIRS, mkw)), mode)
    assert_same(got, run_packed(reg, pkg, tab, P.PAIRS, mp), mode)
    assert not got["count"][:, 1].any() and got["count"][:, 0].max() > 0
    # the host form: the same bytes
    corr, d2, count, slot = reg.match_pairs(tab["feat"], tab["set_off"], P.PAIRS, mp)
    assert all_bytes(dict(slot=slot.astype(np.int64), corr=corr, d2=d2, count=count)) == all_bytes(got), mode


# ---- 2: match + registration -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["weight_count", "degree_count", "weight_mse"])
def test_register_pairs_features_equals_both_comparators(pkg, O, reg, cfg):
    rank_mode, score_mode = dict(weight_count=(0, 0), degree_count=(1, 0), weight_mse=(0, 1))[cfg]
    tab = P.table()
    kw = dict(P.KW, rank_mode=rank_mode)
    mp = pkg.api.make_match_params(P.DIM, **MUTUAL)
    p = pkg.make_params(**kw, score_mode=score_mode)
    got = run_pairs(reg, pkg, tab, P.PAIRS, mp, p)
    ref = _ref(("features", cfg), lambda: P.features(O, tab, P.PAIRS, MUTUAL, kw, score_mode))
    assert_features_ref(got, ref, cfg)
    assert_same(got, run_packed(reg, pkg, tab, P.PAIRS, mp, p), cfg)
    statuses = got["res"]["status"].tolist()
    assert SC_OK in statuses and SC_ENOHYP in statuses and (got["count"][:, 0] < 3).any()
    # the points' layout does not matter
    soa = run_pairs(reg, pkg, tab, P.PAIRS, mp, pkg.make_params(**kw, score_mode=score_mode, layout=pkg.SC_SOA))
    assert all_bytes(soa) == all_bytes(got), cfg
    # the host form agrees with the device form
    res, corr, d2, count, mask, slot = reg.register_pairs_features(tab["pts"], tab["feat"], tab["set_off"], P.PAIRS, mp, p)
    assert all_bytes(dict(slot=slot.astype(np.int64), corr=corr, d2=d2, count=count, res=res, mask=mask)) == all_bytes(got), cfg


# ---- 3: the polish behind it -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [1, 16])
def test_polish_pairs_slots_equals_both_comparators(pkg, O, reg, max_iter):
    tab = P.table()
    mp = pkg.api.make_match_params(P.DIM, **MUTUAL)
    q = pkg.make_polish_params(candidates=1, max_iter=max_iter)
    feats = _ref(("features", "tau 0.02"), lambda: P.features(O, tab, P.PAIRS, MUTUAL, KW02))
    ref = _ref(("polish", max_iter), lambda: P.polish(O, tab, P.PAIRS, feats, 0.02, 0, max_iter))
    seen = None
    for soa in (False, True):
        p = pkg.make_params(**KW02, layout=pkg.SC_SOA if soa else pkg.SC_AOS)
        got = run_pairs(reg, pkg, tab, P.PAIRS, mp, p, q)
        print(max_iter, soa, [tuple(int(o[f]) for f in PB.FIELDS) for o in got["pol"]])
        assert_features_ref(got, feats, f"polish input {max_iter}")
        assert_polish_ref(got, ref, f"polish {max_iter} soa={soa}")
        assert_same(got, run_packed(reg, pkg, tab, P.PAIRS, mp, p, q), f"polish {max_iter} soa={soa}")
        seen = seen or all_bytes(got)
        assert all_bytes(got) == seen
    assert int(got["pol"]["iters"].max()) >= 1
    for pr in range(len(P.PAIRS)):  # a short pair passes its status through
        if got["count"][pr, 0] < 3:
            assert int(got["pol"][pr]["status"]) == SC_ENOHYP and got["pol"][pr]["Rt"].tobytes() == batch_ref.IDENT.tobytes()


# ---- 4: a pair's outputs are a function of its two sets and the parameters ----------------------------------------------------------
def test_permuting_and_embedding_the_list(pkg, reg):
    tab = P.table()
    mp = pkg.api.make_match_params(P.DIM, **MUTUAL)
    p = pkg.make_params(**P.KW)
    q = pkg.make_polish_params(candidates=1, max_iter=16)
    n = len(P.PAIRS)
    base = all_bytes(run_pairs(reg, pkg, tab, P.PAIRS, mp, p, q))
    for order in (list(range(n))[::-1], [(k * 7 + 3) % n for k in range(n)]):
        assert sorted(order) == list(range(n))
        got = all_bytes(run_pairs(reg, pkg, tab, P.PAIRS[order], mp, p, q))
        assert got == [base[k] for k in order], order
    head = np.array([(P.R129, P.R129), (P.R1, P.R1), (P.scene_tgt(4), P.scene_src(4))], np.uint32)
    tail = np.array([(P.R65, P.R65), (P.TIE_B, P.TIE_A)], np.uint32)
    longer = all_bytes(run_pairs(reg, pkg, tab, np.concatenate([head, P.PAIRS, tail]), mp, p, q))
    assert longer[len(head): len(head) + n] == base
    # two pairs that share a target set under mutual matching, next to each other and alone
    for k in range(n):
        assert all_bytes(run_pairs(reg, pkg, tab, P.PAIRS[k: k + 1], mp, p, q))[0] == base[k], k


# ---- 5: a non-finite descriptor flags the pairs of its set -----------------------------------------------------------------------------
def test_a_nan_in_one_set_flags_exactly_its_pairs(pkg, reg):
    tab = P.table()
    pts, feat = tab["sets"][P.R65]
    bad = feat.copy(); bad[-1, -1] = np.nan  # the last component of the last row: the second row tile, the short chunk
    dirty = P.with_sets(tab, {P.R65: (pts, bad)})
    mp = pkg.api.make_match_params(P.DIM, **MUTUAL)
    p = pkg.make_params(**P.KW)
    base = run_pairs(reg, pkg, tab, P.PAIRS, mp, p)
    got = run_pairs(reg, pkg, dirty, P.PAIRS, mp, p)  # (returns: the call's status is SC_OK)
    uses = [P.R65 in ab for ab in P.PAIRS.tolist()]
    assert sum(uses) >= 6 and not all(uses)
    assert got["count"][:, 1].tolist() == [1 if u else 0 for u in uses]
    for k, u in enumerate(uses):
        if u:
            r = got["res"][k]
            assert got["count"][k, 0] == 0 and int(r["status"]) == SC_EINVAL and int(r["n"]) == 0, k
            assert r["Rt"].tobytes() == batch_ref.IDENT.tobytes() and [int(r[f]) for f in FIELDS[2:]] == [0] * 5, k
        else:
            assert pair_bytes(got, k) == pair_bytes(base, k), k
    assert_same(got, run_packed(reg, pkg, dirty, P.PAIRS, mp, p), "nan")


# ---- 6: what is refused with a context, and that nothing is enqueued ---------------------------------------------------------------
def test_refusals_name_the_rule_and_enqueue_nothing(pkg, reg):
    import torch
    tab = P.table()
    off = tab["set_off"]
    mk = pkg.api.make_match_params
    p = pkg.make_params(**P.KW)
    q = pkg.make_polish_params(candidates=1, max_iter=4)
    d_feat = torch.from_numpy(tab["feat"]).cuda(); d_pts = torch.from_numpy(tab["pts"]).cuda()
    o = _outputs(torch, 4, 4 * 257 * 2, True, True)
    before = {k: v.clone() for k, v in o.items()}
    torch.cuda.synchronize()

    def match(pairs, mp, set_off=off):
        reg.match_pairs_device(d_feat.data_ptr(), set_off, pairs, mp, o["corr"].data_ptr(), o["d2"].data_ptr(), o["count"].data_ptr())

    def features(pairs, mp, pp=p, set_off=off):
        reg.register_pairs_features_device(d_pts.data_ptr(), d_feat.data_ptr(), set_off, pairs, mp, pp, o["res"].data_ptr(), o["corr"].data_ptr(),
                                           o["d2"].data_ptr(), o["count"].data_ptr(), o["mask"].data_ptr())

    def polish(pairs, knn, qq=q):
        reg.polish_pairs_slots_device(d_pts.data_ptr(), off, pairs, knn, p, qq, o["corr"].data_ptr(), o["count"].data_ptr(), o["res"].data_ptr(),
                                      o["pol"].data_ptr(), o["pmask"].data_ptr())

    dec = off.copy(); dec[P.EMPTY] = dec[P.EMPTY - 1] - 1  # a decrease between two sets no pair names
    cases = {
        "a set index == n_sets": (lambda: match([(P.R2, P.N_SETS)], mk(P.DIM)), ">= n_sets"),
        "a set index of all ones (features)": (lambda: features([(0xFFFFFFFF, P.R2)], mk(P.DIM)), ">= n_sets"),
        "a referenced empty source": (lambda: match([(P.R2, P.R3), (P.EMPTY, P.R2)], mk(P.DIM)), "no rows"),
        "a referenced empty target (features)": (lambda: features([(P.R2, P.EMPTY)], mk(P.DIM)), "no rows"),
        "n_pairs == 0": (lambda: match(np.zeros((0, 2), np.uint32), mk(P.DIM)), "n_pairs"),
        "set_off decreasing": (lambda: match([(P.R2, P.R3)], mk(P.DIM), dec), "decreases"),
        "ns * knn = 514 (features)": (lambda: features([(P.R257, P.R2)], mk(P.DIM, knn=2)), "SC_BATCH_MAX_N"),
        "ns * knn = 514 (polish)": (lambda: polish([(P.R257, P.R2)], 2), "SC_BATCH_MAX_N"),
        "knn = 5": (lambda: match([(P.R2, P.R3)], mk(P.DIM, knn=5)), "knn"),
        "polish: knn = 0": (lambda: polish([(P.R2, P.R3)], 0), "knn"),
        "mutual with knn = 2": (lambda: match([(P.R2, P.R3)], mk(P.DIM, knn=2, mutual=True)), "knn == 1"),
        "shard_world = 2": (lambda: features([(P.R2, P.R3)], mk(P.DIM), pkg.make_params(**P.KW, shard_world=2)), "shard_world"),
        "SC_FLAG_REFINE": (lambda: features([(P.R2, P.R3)], mk(P.DIM), pkg.make_params(**P.KW, flags=8)), "sc_register_pairs_features"),
        "polish: candidates = 8": (lambda: polish([(P.R2, P.R3)], 1, pkg.make_polish_params()), "candidates"),
        "polish: max_iter = 65": (lambda: polish([(P.R2, P.R3)], 1, pkg.make_polish_params(candidates=1, max_iter=65)), "max_iter"),
    }
    for what, (call, word) in cases.items():
        with pytest.raises(pkg.SacCotError) as e:
            call()
        err = reg._lib.sc_last_error(reg._h).decode()
        print(what, e.value.status, err)
        assert e.value.status == SC_EINVAL and word in err, what
    # a NULL argument with a context: named
    rc = reg._lib.sc_match_pairs_device(reg._h, d_feat.data_ptr(), off.ctypes.data_as(C.POINTER(C.c_uint32)), P.N_SETS, None, 1,
                                        C.byref(mk(P.DIM)), 64, 64, 64)
    assert rc == SC_EINVAL and "NULL" in reg._lib.sc_last_error(reg._h).decode()
    # a call outstanding on the context
    s, t = batch_ref.scene(pkg, 128, .3)
    d_s, d_t = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
    d_rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_m = torch.zeros(128, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reg.register_device_async(d_s.data_ptr(), d_t.data_ptr(), 128, p, d_rt.data_ptr(), d_m.data_ptr())
    for call in (lambda: match([(P.R2, P.R3)], mk(P.DIM)), lambda: features([(P.R2, P.R3)], mk(P.DIM)), lambda: polish([(P.R2, P.R3)], 1)):
        with pytest.raises(pkg.SacCotError) as e:
            call()
        assert e.value.status == SC_EINVAL and "outstanding" in reg._lib.sc_last_error(reg._h).decode()
    rc, _ = reg.wait()
    assert rc == SC_OK
    torch.cuda.synchronize()
    for k, v in o.items():  # nothing was enqueued: no output moved
        assert torch.equal(v, before[k]), k
    # the match alone takes what the features entries refuse for the slot bound; the context stays usable
    match([(P.R257, P.R2)], mk(P.DIM, knn=2))
    torch.cuda.synchronize()
    assert o["count"][0].tolist() == [514, 0]


# ---- 7, 8: what the calls leave ------------------------------------------------------------------------------------------------------
def test_every_entry_ends_the_frame(pkg, reg):
    import torch
    tab = P.table()
    pairs = P.PAIRS[:4]
    mp = pkg.api.make_match_params(P.DIM, **MUTUAL)
    p = pkg.make_params(**P.KW)
    q = pkg.make_polish_params(candidates=1, max_iter=2)
    s, t = batch_ref.scene(pkg, 128, .3)
    calls = (lambda: reg.match_pairs(tab["feat"], tab["set_off"], pairs, mp),
             lambda: run_pairs(reg, pkg, tab, pairs, mp),
             lambda: reg.register_pairs_features(tab["pts"], tab["feat"], tab["set_off"], pairs, mp, p),
             lambda: run_pairs(reg, pkg, tab, pairs, mp, p),
             lambda: run_pairs(reg, pkg, tab, pairs, mp, p, q))
    for call in calls:
        assert reg.register(s, t, params=p)["status"] == SC_OK  # a frame ...
        call()
        torch.cuda.synchronize()
        with pytest.raises(pkg.SacCotError) as e:  # ... is gone
            reg.peel()
        assert e.value.status == SC_EINVAL


def test_workspace_grows_on_the_first_call_only(pkg):
    r = pkg.Registrar(0)
    try:
        tab = P.table()
        mp = pkg.api.make_match_params(P.DIM, **MUTUAL)
        s, t = batch_ref.scene(pkg, 128, .3)
        p = pkg.make_params(**P.KW)
        ws = lambda: r.register(s, t, params=p)["stats"]["workspace_bytes"]  # noqa: E731
        first = ws()
        assert ws() == first  # sc_register alone: it does not move
        run_pairs(r, pkg, tab, P.PAIRS, mp, p)
        second = ws()
        run_pairs(r, pkg, tab, P.PAIRS, mp, p)
        run_pairs(r, pkg, tab, P.PAIRS[::-1], mp, p)
        third = ws()
        print(first, second, third)
        assert second > first and third == second
    finally:
        r.close()
