"""GPU: descriptor matching for a whole batch of small problems (include/saccot.h, sc_match_batch* / sc_register_batch_features*).

The expected value of every case is tests/match_batch_ref.py — per problem the canonical matcher in numpy float32, a gather, and the
CPU restatement's whole path — and everything is compared bit for bit: every correspondence, the bits of every distance, every
count pair, every field of every record and every mask byte.  No tolerances.  The scenes are checked on the CPU by
tests/test_match_batch_abi.py (at most batch_ref.TRI_CAP triangles a problem, so no workgroup runs long).
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref
import match_batch_ref as M
from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
SC_FLAG_TIMING, SC_FLAG_EXACT_TOTAL, SC_FLAG_REFINE, SC_FLAG_EST_BOUND, SC_FLAG_SHARD_AB = 1, 2, 8, 128, 4096
FIELDS = ("status", "n", "edges", "tri_kept", "tri_total", "best_rank", "best_count")

_REF = {}


def _ref_match(tag, problems, mkw):
    """the reference of a set of problems under one mode, once per session; never modified"""
    key = (tag, tuple(sorted(mkw.items())))
    if key not in _REF:
        _REF[key] = [M.match_one(a, b, **mkw) for a, b in problems]
    return _REF[key]


def _ref_features(O, tag, scenes, mkw):
    key = ("features", tag, tuple(sorted(mkw.items())))
    if key not in _REF:
        _REF[key] = [M.features_one(O, s[0], s[1], s[2], s[3], mkw, M.KW) for s in scenes]
    return _REF[key]


def _slot_bytes(o):
    return (o["n"], o["nonfinite"], o["corr"].tobytes(), o["d2"].tobytes())


def _assert_match(got, exp, what):
    assert len(got) == len(exp), what
    for b, (g, (corr, d2, n, flag)) in enumerate(zip(got, exp)):
        assert (g["n"], int(g["nonfinite"])) == (n, flag), (what, b, g["n"], n)
        assert np.array_equal(g["corr"], corr), (what, b)
        assert g["d2"].tobytes() == d2.tobytes(), (what, b)


def _assert_solo(reg, got, problems, mkw, what):
    """every slot equals sc_match on the problem alone"""
    for b, (a, t) in enumerate(problems):
        solo = reg.match(a, t, **mkw)
        assert got[b]["n"] == solo["n"] and np.array_equal(got[b]["corr"], solo["corr"]), (what, b)
        assert got[b]["d2"].tobytes() == solo["d2"].tobytes(), (what, b)


# ---- 1: the mixed batch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", M.MIXED_DIMS)
def test_mixed_batch_equals_the_reference_and_sc_match(reg, dim):
    assert any(ns == M.ROW_TILE - 1 for ns, _ in M.MIXED_SIZES) and any(ns == M.ROW_TILE + 1 for ns, _ in M.MIXED_SIZES)
    problems = M.mixed_descriptors(dim)
    for mkw in M.MATCH_MODES:
        got = reg.match_batch(problems, **mkw)
        print(dim, mkw, [g["n"] for g in got])
        _assert_match(got, _ref_match(("mixed", dim), problems, mkw), (dim, mkw))
        _assert_solo(reg, got, problems, mkw, (dim, mkw))


def test_one_small_problem_at_dim_1024(reg):
    rng = np.random.default_rng(1024)
    problems = [(rng.normal(size=(5, 1024)).astype(np.float32), rng.normal(size=(7, 1024)).astype(np.float32))]
    for mkw in M.MATCH_MODES:
        got = reg.match_batch(problems, **mkw)
        _assert_match(got, _ref_match("d1024", problems, mkw), mkw)
        _assert_solo(reg, got, problems, mkw, mkw)


# ---- 2: ties: the index alone decides ----------------------------------------------------------------------------------------------
def test_ties_are_decided_by_index(reg):
    problems = M.tie_descriptors()
    for mkw in M.MATCH_MODES:
        got = reg.match_batch(problems, **mkw)
        _assert_match(got, _ref_match("ties", problems, mkw), mkw)
        _assert_solo(reg, got, problems, mkw, mkw)
    one = reg.match_batch(problems, knn=1)  # a tied minimum goes to the lowest target index
    for (a, b), g in zip(problems, one):
        for i, j in g["corr"]:
            assert not (b[:j] == b[j]).all(axis=1).any()


# ---- 3: sums that overflow to +inf next to ordinary ones ---------------------------------------------------------------------------
def test_distances_that_overflow(reg):
    rng = np.random.default_rng(3)
    problems = []
    for ns, nt in ((6, 9), (70, 65)):
        a = rng.normal(size=(ns, 5)).astype(np.float32); b = rng.normal(size=(nt, 5)).astype(np.float32)
        a[::2, 1] = 1e20; b[::3, 1] = -1e20; b[1::3, 1] = 1e20  # (1e20 - -1e20)^2 = +inf; 1e20 against an ordinary row: 1e40 = +inf too
        problems.append((a, b))
    problems.append(M.mixed_descriptors(5, ((20, 30),))[0])
    for mkw in M.MATCH_MODES:
        got = reg.match_batch(problems, **mkw)
        exp = _ref_match("overflow", problems, mkw)
        _assert_match(got, exp, mkw)
        _assert_solo(reg, got, problems, mkw, mkw)
    assert np.isinf(_ref_match("overflow", problems, dict(knn=4))[0][1]).any()  # the overflow is really there


# ---- 4: a non-finite descriptor flags its own problem ------------------------------------------------------------------------------
def test_non_finite_descriptors_flag_their_own_problem(reg):
    clean = M.mixed_descriptors(17)
    dirty = [(a.copy(), b.copy()) for a, b in clean]
    dirty[9][0][-1, -1] = np.nan   # the last component of the last source row (129 rows: the third row tile)
    dirty[4][1][-1, 2] = np.inf    # the last target row (65 rows: the second column tile)
    for mkw in (dict(knn=1), dict(knn=3), dict(knn=1, mutual=True, ratio=0.8)):
        base = reg.match_batch(clean, **mkw)
        got = reg.match_batch(dirty, **mkw)
        assert [int(g["nonfinite"]) for g in got] == [1 if b in (4, 9) else 0 for b in range(len(clean))], mkw
        _assert_match(got, [M.match_one(a, b, **mkw) for a, b in dirty], mkw)
        for b in range(len(clean)):
            if b in (4, 9):
                assert got[b]["n"] == 0
            else:
                assert _slot_bytes(got[b]) == _slot_bytes(base[b]), (mkw, b)


# ---- 5: a slot is a function of its own problem and the parameters -----------------------------------------------------------------
def test_independence_of_position_neighbours_and_history(reg):
    problems = M.mixed_descriptors(33)
    nb = len(problems)
    for mkw in (dict(knn=2), dict(knn=1, mutual=True)):
        base = [_slot_bytes(o) for o in reg.match_batch(problems, **mkw)]
        for order in (list(range(nb))[::-1], [(b + 4) % nb for b in range(nb)], list(range(nb))):
            got = reg.match_batch([problems[b] for b in order], **mkw)
            assert [_slot_bytes(o) for o in got] == [base[b] for b in order], (mkw, order)
        for b in range(nb):
            assert _slot_bytes(reg.match_batch([problems[b]], **mkw)[0]) == base[b], (mkw, b)


# ---- 6: what is refused ----------------------------------------------------------------------------------------------------------
def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _raw_match(reg, so, to, nb, mp, dim=4):
    """sc_match_batch called directly on descriptors of the offsets' own totals (capped: a refused call reads none) -> (rc, error)"""
    f = np.zeros((min(int(max(so[-1], to[-1])), 8192) + 1, dim), np.float32)
    slots = min(int(so[-1]) * 4, 1 << 16) + 1
    corr = np.zeros((slots, 2), np.int32); d2 = np.zeros(slots, np.float32); cnt = np.zeros((max(nb, 1), 2), np.uint32)
    rc = reg._lib.sc_match_batch(reg._h, _ptr(f, C.c_float), _ptr(so, C.c_uint32), _ptr(f, C.c_float), _ptr(to, C.c_uint32), nb, C.byref(mp),
                                 _ptr(corr, C.c_int32), _ptr(d2, C.c_float), _ptr(cnt, C.c_uint32))
    return rc, reg._lib.sc_last_error(reg._h).decode()


def _raw_features(reg, so, to, nb, mp, p, dim=4):
    n = int(max(so[-1], to[-1])) + 1
    f = np.zeros((n, dim), np.float32); pts = np.zeros((n, 3), np.float32)
    slots = int(so[-1]) * 4 + 1
    corr = np.zeros((slots, 2), np.int32); d2 = np.zeros(slots, np.float32); cnt = np.zeros((max(nb, 1), 2), np.uint32)
    res = np.zeros(max(nb, 1), batch_ref.RESULT_DTYPE); mask = np.zeros(slots, np.uint8)
    rc = reg._lib.sc_register_batch_features(reg._h, _ptr(pts, C.c_float), _ptr(f, C.c_float), _ptr(so, C.c_uint32), _ptr(pts, C.c_float),
                                             _ptr(f, C.c_float), _ptr(to, C.c_uint32), nb, C.byref(mp), C.byref(p),
                                             res.ctypes.data_as(C.c_void_p), _ptr(corr, C.c_int32), _ptr(d2, C.c_float),
                                             _ptr(cnt, C.c_uint32), _ptr(mask, C.c_uint8))
    return rc, reg._lib.sc_last_error(reg._h).decode()


def test_refusals_leave_the_context_usable(pkg, reg):
    import torch
    u32 = lambda *a: np.array(a, np.uint32)  # noqa: E731
    mk = pkg.api.make_match_params
    good_problem = M.mixed_descriptors(4, ((20, 30),))
    good = _slot_bytes(reg.match_batch(good_problem, knn=2)[0])
    ok = u32(0, 8, 16)
    bad_size = mk(4); bad_size.size = 8
    reserved = mk(4); reserved.reserved[1] = 1
    big = (np.arange((1 << 19) + 2, dtype=np.uint64) * 4096).astype(np.uint64)
    cases = {
        "n_problems = 0": (u32(0), u32(0), 0, mk(4), "n_problems"),
        "ns_b = 0": (u32(0, 8, 8), ok, 2, mk(4), "no rows"),
        "nt_b = 0": (ok, u32(0, 8, 8), 2, mk(4), "no rows"),
        "ns_b = 4097": (u32(0, 4097), u32(0, 8), 1, mk(4), "SC_MATCH_BATCH_MAX_N"),
        "nt_b = 4097": (u32(0, 8), u32(0, 4097), 1, mk(4), "SC_MATCH_BATCH_MAX_N"),
        "source offsets decrease": (u32(0, 64, 60, 128), u32(0, 8, 16, 24), 3, mk(4), "decrease"),
        "target offsets decrease": (u32(0, 8, 16, 24), u32(0, 64, 60, 128), 3, mk(4), "decrease"),
        "total_s * knn > 2^31": (big[: (1 << 17) + 2].astype(np.uint32), np.arange((1 << 17) + 2, dtype=np.uint32), (1 << 17) + 1, mk(4, knn=4), "2^31"),
        "knn = 5": (ok, ok, 2, mk(4, knn=5), "knn"),
        "dim = 0": (ok, ok, 2, mk(0), "dim"),
        "dim = 1025": (ok, ok, 2, mk(1025), "dim"),
        "mutual with knn = 2": (ok, ok, 2, mk(4, knn=2, mutual=True), "knn == 1"),
        "ratio with knn = 2": (ok, ok, 2, mk(4, knn=2, ratio=0.5), "knn == 1"),
        "ratio = 1": (ok, ok, 2, mk(4, ratio=1.0), "ratio"),
        "an unknown flag": (ok, ok, 2, mk(4, flags=2), "flags"),
        "a reserved word": (ok, ok, 2, reserved, "reserved"),
        "sc_match_params.size": (ok, ok, 2, bad_size, "size"),
    }
    for what, (so, to, nb, mp, word) in cases.items():
        rc, err = _raw_match(reg, so, to, nb, mp)
        print(what, rc, err)
        assert rc == SC_EINVAL and word in err, what
        assert _slot_bytes(reg.match_batch(good_problem, knn=2)[0]) == good, what  # the context stays usable
    # the features entries refuse all of that (one is tried) and what is their own
    kw = M.KW
    fcases = {
        "a decreasing offset": (u32(0, 64, 60, 128), u32(0, 8, 16, 24), 3, mk(4), pkg.make_params(**kw), "decrease"),
        "ns_b * knn = 514": (u32(0, 257), u32(0, 300), 1, mk(4, knn=2), pkg.make_params(**kw), "SC_BATCH_MAX_N"),
        "shard_world = 2": (ok, ok, 2, mk(4), pkg.make_params(**kw, shard_world=2), "shard_world"),
        "SC_FLAG_REFINE": (ok, ok, 2, mk(4), pkg.make_params(**kw, flags=SC_FLAG_REFINE), "sc_register_batch_features"),
        "SC_FLAG_TIMING": (ok, ok, 2, mk(4), pkg.make_params(**kw, flags=SC_FLAG_TIMING), "sc_register_batch_features"),
        "SC_FLAG_EST_BOUND": (ok, ok, 2, mk(4), pkg.make_params(**kw, flags=SC_FLAG_EST_BOUND), "sc_register_batch_features"),
        "SC_FLAG_SHARD_AB": (ok, ok, 2, mk(4), pkg.make_params(**kw, flags=SC_FLAG_SHARD_AB), "sc_register_batch_features"),
        "bad sc_params": (ok, ok, 2, mk(4), pkg.make_params(**dict(kw, tau=-1.0)), "sc_params"),
    }
    for what, (so, to, nb, mp, p, word) in fcases.items():
        rc, err = _raw_features(reg, so, to, nb, mp, p)
        print(what, rc, err)
        assert rc == SC_EINVAL and word in err, what
    # a NULL argument with a context: named
    f = np.zeros((16, 4), np.float32); cnt = np.zeros((2, 2), np.uint32)
    rc = reg._lib.sc_match_batch(reg._h, _ptr(f, C.c_float), _ptr(ok, C.c_uint32), _ptr(f, C.c_float), None, 2, C.byref(mk(4)), None, None,
                                 _ptr(cnt, C.c_uint32))
    assert rc == SC_EINVAL and "NULL" in reg._lib.sc_last_error(reg._h).decode()
    rc = reg._lib.sc_match_batch_device(reg._h, 64, _ptr(ok, C.c_uint32), 64, _ptr(ok, C.c_uint32), 2, None, 64, 64, 64)
    assert rc == SC_EINVAL and "NULL" in reg._lib.sc_last_error(reg._h).decode()
    # a call outstanding on the context
    s, t = batch_ref.scene(pkg, 128, .3)
    d_s, d_t = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
    d_rt = torch.zeros(12, dtype=torch.float32, device="cuda"); d_m = torch.zeros(128, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = pkg.make_params(**kw)
    reg.register_device_async(d_s.data_ptr(), d_t.data_ptr(), 128, p, d_rt.data_ptr(), d_m.data_ptr())
    rc, err = _raw_match(reg, ok, ok, 2, mk(4))
    assert rc == SC_EINVAL and "outstanding" in err
    rc, err = _raw_features(reg, ok, ok, 2, mk(4), p)
    assert rc == SC_EINVAL and "outstanding" in err
    rc, _ = reg.wait()
    assert rc == SC_OK
    assert _slot_bytes(reg.match_batch(good_problem, knn=2)[0]) == good


# ---- 7: sc_register_batch_features ---------------------------------------------------------------------------------------------------
def _assert_features(got, exp, what):
    assert len(got) == len(exp), what
    for b, (g, e) in enumerate(zip(got, exp)):
        er = e["rec"]
        print(what, b, "n", g["n"], [g["status"]] + [g["stats"][f] for f in FIELDS[1:]], "| expected", [int(er[f]) for f in FIELDS])
        assert g["n"] == e["n"] and np.array_equal(g["corr"], e["corr"]) and g["d2"].tobytes() == e["d2"].tobytes(), (what, b)
        assert [g["status"]] + [g["stats"][f] for f in FIELDS[1:]] == [int(er[f]) for f in FIELDS], (what, b)
        assert nan_equal_bits(np.concatenate([g["R"].ravel(), g["t"]]), er["Rt"]), (what, b)
        assert np.array_equal(g["mask"], e["mask"]), (what, b)


@pytest.mark.parametrize("mode", ["mutual", "knn2"])
def test_register_batch_features_equals_the_composition(pkg, O, reg, mode):
    mkw = dict(knn=1, mutual=True) if mode == "mutual" else dict(knn=2)
    scenes = M.feature_scenes()
    problems = [s[:4] for s in scenes]
    exp = _ref_features(O, "scenes", scenes, mkw)
    aos = reg.register_batch_features(problems, params=pkg.make_params(**M.KW), **mkw)
    _assert_features(aos, exp, f"AoS {mode}")
    soa = reg.register_batch_features(problems, params=pkg.make_params(**M.KW, layout=pkg.SC_SOA), **mkw)
    _assert_features(soa, exp, f"SoA {mode}")
    statuses = [o["status"] for o in aos]
    assert SC_OK in statuses and SC_ENOHYP in statuses
    solo_p = pkg.make_params(**M.KW, flags=SC_FLAG_EXACT_TOTAL)
    for b, (o, s) in enumerate(zip(aos, problems)):  # an SC_OK problem equals sc_register_features on it alone
        if o["status"] != SC_OK:
            continue
        solo = reg.register_features(s[0], s[1], s[2], s[3], params=solo_p, **mkw)
        st = solo["stats"]
        assert solo["status"] == SC_OK and solo["n"] == o["n"] and np.array_equal(solo["corr"], o["corr"]), b
        assert nan_equal_bits(solo["R"], o["R"]) and nan_equal_bits(solo["t"], o["t"]) and np.array_equal(solo["mask"], o["mask"]), b
        assert [st[f] for f in ("edges", "tri_kept", "tri_total", "best_rank", "best_count")] == \
               [o["stats"][f] for f in ("edges", "tri_kept", "tri_total", "best_rank", "best_count")], b


def test_features_non_finite_descriptor_and_point(pkg, O, reg):
    scenes = M.feature_scenes()
    problems = [list(s[:4]) for s in scenes[3:6]]
    problems[0][1] = problems[0][1].copy(); problems[0][1][0, 0] = np.inf          # a descriptor: the flag, SC_EINVAL, n = 0
    exp_mid = M.features_one(O, *problems[1], dict(knn=1, mutual=True), M.KW)
    i0 = int(exp_mid["corr"][0, 0])
    problems[1][0] = problems[1][0].copy(); problems[1][0][i0, 1] = np.nan          # a matched point: SC_EINVAL, n = n_b
    mkw = dict(knn=1, mutual=True)
    exp = [M.features_one(O, *p, mkw, M.KW) for p in problems]
    assert [int(e["rec"]["status"]) for e in exp] == [SC_EINVAL, SC_EINVAL, SC_OK] and exp[0]["rec"]["n"] == 0 and exp[1]["rec"]["n"] == exp[1]["n"]
    got = reg.register_batch_features([tuple(p) for p in problems], params=pkg.make_params(**M.KW), **mkw)
    _assert_features(got, exp, "non-finite")


# ---- 8: the device forms; what the calls leave -----------------------------------------------------------------------------------
def test_device_forms_equal_host_forms(pkg, O, reg):
    import torch
    scenes = M.feature_scenes()
    problems = [s[:4] for s in scenes]
    mp = pkg.api.make_match_params(33, mutual=True)
    p = pkg.make_params(**M.KW)
    so = reg._offsets([len(s[1]) for s in problems]); to = reg._offsets([len(s[3]) for s in problems])
    src, fsrc = np.concatenate([s[0] for s in problems]), np.concatenate([s[1] for s in problems])
    tgt, ftgt = np.concatenate([s[2] for s in problems]), np.concatenate([s[3] for s in problems])
    nb, slots = len(problems), int(so[-1])
    h_res, h_corr, h_d2, h_count, h_mask = reg.register_batch_features_raw(src, fsrc, so, tgt, ftgt, to, mp, p)
    m_corr, m_d2, m_count = reg.match_batch_raw(fsrc, so, ftgt, to, mp)
    assert np.array_equal(m_count, h_count)

    def valid(arr, count, width=1):
        """the specified part of a slot array: the first n_b entries of every slot"""
        return b"".join(arr[int(so[b]): int(so[b]) + int(count[b, 0])].tobytes() for b in range(nb))

    assert valid(m_corr, m_count) == valid(h_corr, h_count) and valid(m_d2, m_count) == valid(h_d2, h_count)
    # the plain batch entry on this context, before: what it returns must not move
    pairs = batch_ref.mixed(pkg)[:5]
    plain = reg.register_batch(pairs, params=p)
    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(src=src, fsrc=fsrc, tgt=tgt, ftgt=ftgt).items()}
    outs = []
    for _ in range(2):
        outs.append(dict(res=torch.zeros(nb * 80, dtype=torch.uint8, device="cuda"), corr=torch.full((slots, 2), -7, dtype=torch.int32, device="cuda"),
                         d2=torch.zeros(slots, dtype=torch.float32, device="cuda"), count=torch.full((nb, 2), 9, dtype=torch.int32, device="cuda"),
                         mask=torch.full((slots,), 7, dtype=torch.uint8, device="cuda")))
    m_out = dict(corr=torch.full((slots, 2), -7, dtype=torch.int32, device="cuda"), d2=torch.zeros(slots, dtype=torch.float32, device="cuda"),
                 count=torch.full((nb, 2), 9, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    reg.set_stream(stream.cuda_stream)
    try:
        for o in outs:  # twice in a row, nothing synchronised in between
            reg.register_batch_features_device(dev["src"].data_ptr(), dev["fsrc"].data_ptr(), so, dev["tgt"].data_ptr(), dev["ftgt"].data_ptr(), to,
                                               mp, p, o["res"].data_ptr(), o["corr"].data_ptr(), o["d2"].data_ptr(), o["count"].data_ptr(),
                                               o["mask"].data_ptr())
        reg.match_batch_device(dev["fsrc"].data_ptr(), so, dev["ftgt"].data_ptr(), to, mp, m_out["corr"].data_ptr(), m_out["d2"].data_ptr(),
                               m_out["count"].data_ptr())
        stream.synchronize()
    finally:
        reg.set_stream(None)
    for o in outs:
        count = o["count"].cpu().numpy().astype(np.uint32)
        assert np.array_equal(count, h_count)
        assert o["res"].cpu().numpy().tobytes() == h_res.tobytes()
        assert valid(o["corr"].cpu().numpy(), count) == valid(h_corr, h_count) and valid(o["d2"].cpu().numpy(), count) == valid(h_d2, h_count)
        assert valid(o["mask"].cpu().numpy(), count) == valid(h_mask, h_count)
    count = m_out["count"].cpu().numpy().astype(np.uint32)
    assert np.array_equal(count, h_count) and valid(m_out["corr"].cpu().numpy(), count) == valid(h_corr, h_count)
    assert valid(m_out["d2"].cpu().numpy(), count) == valid(h_d2, h_count)
    # sc_register_batch on the same context: unchanged
    again = reg.register_batch(pairs, params=p)
    for a, b in zip(plain, again):
        assert a["status"] == b["status"] and a["stats"] == b["stats"] and np.array_equal(a["mask"], b["mask"])
        assert a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes()
    # each of the four ends the frame a context may hold and leaves none
    s, t = batch_ref.scene(pkg, 128, .3)
    desc = [(sc[1], sc[3]) for sc in problems]
    o = outs[0]
    calls = (lambda: reg.match_batch(desc, mutual=True),
             lambda: reg.match_batch_device(dev["fsrc"].data_ptr(), so, dev["ftgt"].data_ptr(), to, mp, m_out["corr"].data_ptr(),
                                            m_out["d2"].data_ptr(), m_out["count"].data_ptr()),
             lambda: reg.register_batch_features(problems, params=p, mutual=True),
             lambda: reg.register_batch_features_device(dev["src"].data_ptr(), dev["fsrc"].data_ptr(), so, dev["tgt"].data_ptr(),
                                                        dev["ftgt"].data_ptr(), to, mp, p, o["res"].data_ptr(), o["corr"].data_ptr(),
                                                        o["d2"].data_ptr(), o["count"].data_ptr(), o["mask"].data_ptr()))
    for call in calls:
        assert reg.register(s, t, params=p)["status"] == SC_OK  # a frame ...
        call()
        torch.cuda.synchronize()
        with pytest.raises(pkg.SacCotError) as e:  # ... is gone
            reg.peel()
        assert e.value.status == SC_EINVAL
        with pytest.raises(pkg.SacCotError) as e:
            reg.polish()
        assert e.value.status == SC_EINVAL


# ---- 9: a context that never calls these entries allocates nothing new -------------------------------------------------------------
def test_workspace_appears_with_the_first_call(pkg):
    r = pkg.Registrar(0)
    try:
        s, t = batch_ref.scene(pkg, 128, .3)
        p = pkg.make_params(**M.KW)
        first = r.register(s, t, params=p)["stats"]["workspace_bytes"]
        assert r.register(s, t, params=p)["stats"]["workspace_bytes"] == first  # sc_register alone: it does not move
        r.match_batch(M.mixed_descriptors(16)[:5], mutual=True)
        second = r.register(s, t, params=p)["stats"]["workspace_bytes"]
        print(first, second)
        assert second > first
    finally:
        r.close()
