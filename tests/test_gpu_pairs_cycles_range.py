"""GPU: sc_pairs_cycles past the first trip of its loops, on its cuts and at the ends of the number range (include/saccot.h).

tests/test_gpu_pairs_cycles.py never hands the entry more pairs than a round's grid has waves (2048 x 4), a neighbour list longer
than a wave, a loop that sits ON a threshold, or a number outside a rotation and a translation in [-1, 1].  These families do
(tests/cycles_ref.py; tests/test_cycles_abi.py checks on the CPU that they are what they are used for):

  k130       8385 pairs: 193 of them take the second trip of the grid-stride loop, every lane loop runs 64 + 64 + 1, and the list
             unravels over 12 rounds with late pairs leaving in nine of them.
  exact24    cube rotations and integer translations: tr in {3, 1, 0, -1}, e2 a small integer, so tr == tr_min and e2 == e2_max
             happen, and an integer evaluation that shares no code with the reference says how many triangles are consistent.
  scaled     the translations and trans_tol times 2^k: everything but max_e2 must not move, and max_e2 moves by 2^(2k) exactly.
  hostile24  finite poses that are no rotations, over the whole exponent range: traces near -1e114, e2 = +inf, -0.0, subnormals.

As there, every comparison is bit for bit — the 48 bytes of every record and the 32 of the summary — against cycles_ref.cycles fed
the thresholds the library derives.  No tolerances.
"""
import numpy as np
import pytest

import cycles_ref as CR
from test_gpu_pairs_cycles import _assert_same, _device, _host, _records

pytestmark = pytest.mark.gpu

INF_BITS = 0x7FF0000000000000
_REF, _GPU0 = {}, {}  # the reference's results, computed once per (family, thresholds, rule) and never written; the GPU's at scale 0


def _params(pkg, f, **kw):
    p = dict(f.params); p.update(kw)
    return pkg.make_cycle_params(**p)


def _expected(pkg, name, f, cp, keep=None):
    """the reference on family `name` (status words that are all SC_OK change nothing: flags is not part of the key)"""
    thr = pkg.cycles_thresholds(cp)
    key = (name, thr, cp.min_ok, cp.max_rounds, keep is not None)
    if key not in _REF:
        _REF[key] = CR.cycles(f.n_sets, f.pairs, f.rt, thr[0], thr[1], min_ok=cp.min_ok, max_rounds=cp.max_rounds, keep=keep)
    return _REF[key]


def _summary(s):
    return tuple(int(s[n]) for n in ("rounds", "stable", "alive", "edges", "triangles", "consistent"))


# ---- k130: the second trip of the grid-stride loop, three trips of the lane loop ----------------------------------------------------
@pytest.mark.parametrize("with_keep", [True, False])
def test_k130_in_every_form(pkg, reg, with_keep):
    f = CR.k130()
    keep = f.keep if with_keep else None
    for stride, flags in ((48, 0), (80, 0), (80, pkg.SC_CYCLES_STATUS)):
        cp = _params(pkg, f, flags=flags)
        exp = _expected(pkg, "k130", f, cp, keep)
        raw = _records(f.rt, stride)
        _assert_same(_device(pkg, reg, f.n_sets, f.pairs, cp, raw, keep=keep), exp, f"device form, stride {stride}, flags {flags}, keep {with_keep}")
        if stride == 80:
            _assert_same(_host(pkg, reg, f.n_sets, f.pairs, cp, raw, keep=keep), exp, f"host form, stride {stride}, flags {flags}, keep {with_keep}")
    _assert_same(reg.pairs_cycles(f.n_sets, f.pairs, f.rt, _params(pkg, f), keep=keep), exp, f"host form, plain poses, keep {with_keep}")
    res, s = exp
    late = np.arange(len(f.pairs)) >= 8192
    if with_keep:
        assert _summary(s) == CR.K130_SUMMARY and np.bincount(res["dropped_round"], minlength=13).tolist() == CR.K130_DROPS
        assert res["alive"][late].sum() == 14 and len(set(res["dropped_round"][late].tolist())) == 10  # 0 (alive), and nine rounds
    else:
        assert _summary(s)[:3] == CR.K130_NO_KEEP and not res["alive"].any() and len(set(res["dropped_round"][late].tolist())) >= 2
    assert (res["cycles"] == 128).all()


def test_k130_cut_short(pkg, reg):
    f = CR.k130()
    cp = _params(pkg, f, max_rounds=CR.K130_SHORT)
    exp = _expected(pkg, "k130", f, cp, f.keep)
    _assert_same(reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp, keep=f.keep), exp, "host form, cut short")
    _assert_same(_device(pkg, reg, f.n_sets, f.pairs, cp, _records(f.rt, 48), keep=f.keep), exp, "device form, cut short")
    assert _summary(exp[1])[:3] == (CR.K130_SHORT, 0, 8385 - sum(CR.K130_DROPS[1:CR.K130_SHORT + 1]))
    assert exp[0]["ok_alive"][exp[0]["dropped_round"] == CR.K130_SHORT].max() > 0  # ok_K of pairs the last round dropped


def test_k130_with_repeated_and_reversed_pairs(pkg, reg):
    f = CR.k130_repeats()
    cp = _params(pkg, f)
    exp = _expected(pkg, "k130_repeats", f, cp, f.keep)
    _assert_same(reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp, keep=f.keep), exp, "repeats, host form")
    _assert_same(_device(pkg, reg, f.n_sets, f.pairs, cp, _records(f.rt, 80), keep=f.keep), exp, "repeats, device form")
    assert _summary(exp[1]) == CR.K130_REPEATS_SUMMARY and exp[0]["cycles"].max() > 128


def test_k130_shuffled(pkg, reg):
    f = CR.k130()
    cp = _params(pkg, f)
    base = reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp, keep=f.keep)
    _assert_same(base, _expected(pkg, "k130", f, cp, f.keep), "k130")
    perm = np.random.default_rng(131).permutation(len(f.pairs))  # other pairs take the second trip
    got = reg.pairs_cycles(f.n_sets, f.pairs[perm], f.rt[perm], cp, keep=f.keep[perm])
    assert got[0].tobytes() == base[0][perm].tobytes() and got[1].tobytes() == base[1].tobytes()


def test_k130_between_small_lists_on_one_context(pkg, reg):
    small, big, k24 = CR.one_triangle(5, True), CR.k130(), CR.k24()
    for name, f in (("one_triangle", small), ("k130", big), ("one_triangle", small), ("k24", k24), ("k130", big), ("k24", k24)):
        cp = _params(pkg, f)
        _assert_same(_device(pkg, reg, f.n_sets, f.pairs, cp, _records(f.rt, 48), keep=f.keep), _expected(pkg, name, f, cp, f.keep), f"{name} in a row")


# ---- exact24: loops that sit on the cuts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot_tol,trans_tol", list(CR.EXACT24_CUTS))
def test_exact24_on_the_cuts(pkg, reg, rot_tol, trans_tol):
    f = CR.exact24()
    tp, tq, tr_, tr, e2 = CR.exact24_integers()
    cp = _params(pkg, f, rot_tol=rot_tol, trans_tol=trans_tol, min_ok=3)
    tr_min, e2_max = pkg.cycles_thresholds(cp)
    good = (tr >= tr_min) & (e2 <= e2_max)  # from the integers
    exp = _expected(pkg, "exact24", f, cp)
    for got, what in ((reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp), "host form"), (_device(pkg, reg, f.n_sets, f.pairs, cp, _records(f.rt, 64)), "device form")):
        _assert_same(got, exp, f"exact24 {rot_tol} {trans_tol}, {what}")
        print("consistent", got[1]["consistent"], "from the integers", good.sum(), "planted", CR.EXACT24_CUTS[(rot_tol, trans_tol)])
        assert got[1]["consistent"] == good.sum() == CR.EXACT24_CUTS[(rot_tol, trans_tol)]
        assert (got[0]["ok"] == sum(np.bincount(role[good], minlength=276) for role in (tp, tq, tr_))).all()
        assert got[0]["max_e2"].max() == e2.max() and got[0]["min_trace"].min() == tr.min() == -1
    if rot_tol == 0.0:  # tr == tr_min on every consistent triangle, and e2 == e2_max on some: both cuts are inclusive
        assert tr_min == 3.0 and e2_max == trans_tol * trans_tol and ((tr == 3) & (e2 == e2_max)).any() and good.sum() == ((tr == 3) & (e2 <= e2_max)).sum()
    if rot_tol == CR.PI32:  # the largest rot_tol there is: a loop off by exactly a half turn is still not consistent
        assert -1.0 < tr_min < -1.0 + 1e-14 and ((tr == -1) & (e2 <= e2_max)).sum() > 0 and good.sum() == ((tr > -1) & (e2 <= e2_max)).sum()


def test_exact24_the_inclusive_cut_is_observable(pkg, reg):
    """from (0, 0) to (0, 1) the consistent triangles strictly grow by those with e2 == 1, and at (0, 0) they are those with tr == 3
    and e2 == 0: a kernel with > or < in place of >= or <= counts 0 at (0, 0)"""
    f = CR.exact24()
    count = [int(reg.pairs_cycles(f.n_sets, f.pairs, f.rt, _params(pkg, f, rot_tol=0.0, trans_tol=t))[1]["consistent"]) for t in (0.0, 1.0, 2.0)]
    assert count == [CR.EXACT24_CUTS[(0.0, t)] for t in (0.0, 1.0, 2.0)] and 0 < count[0] < count[1] < count[2]


# ---- scaled: the exponent range of the translations -----------------------------------------------------------------------------------
def _scale_case(name):
    f = CR.k24() if name == "k24" else CR.k130()
    return f, dict(min_ok=3, max_rounds=16) if name == "k24" else {}


@pytest.mark.parametrize("k", [-140, -100, -40, 40, 100, 120])
@pytest.mark.parametrize("name", ["k24", "k130"])
def test_scaled_translations(pkg, reg, name, k):
    f, kw = _scale_case(name)
    g = CR.scaled(f, k)
    cp = _params(pkg, g, **kw)
    exp = _expected(pkg, f"{name} x 2^{k}", g, cp, g.keep)
    got = _device(pkg, reg, g.n_sets, g.pairs, cp, _records(g.rt, 48), keep=g.keep)
    _assert_same(got, exp, f"{name} x 2^{k}, device form")
    if name == "k24":
        _assert_same(reg.pairs_cycles(g.n_sets, g.pairs, g.rt, cp, keep=g.keep), exp, f"{name} x 2^{k}, host form")
    if abs(k) in (40, 100):  # the covariance, against the GPU's own result at scale 0 (at -140 the floats are subnormal and rounded)
        if name not in _GPU0:
            _GPU0[name] = _device(pkg, reg, f.n_sets, f.pairs, _params(pkg, f, **kw), _records(f.rt, 48), keep=f.keep)
        base, bs = _GPU0[name]
        assert got[1].tobytes() == bs.tobytes()
        for field in base.dtype.names:
            want = np.ldexp(base["max_e2"], 2 * k) if field == "max_e2" else base[field]
            assert got[0][field].tobytes() == want.tobytes(), (name, k, field)
        assert (got[0]["max_e2"] > 0).any()


# ---- hostile24: poses that are no rotations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_ok", [0, 1])
def test_hostile24(pkg, reg, min_ok):
    f = CR.hostile24()
    cp = _params(pkg, f, min_ok=min_ok)
    exp = _expected(pkg, "hostile24", f, cp)
    for got, what in ((reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp), "host form"), (_device(pkg, reg, f.n_sets, f.pairs, cp, _records(f.rt, 48)), "device form"),
                      (_device(pkg, reg, f.n_sets, f.pairs, _params(pkg, f, min_ok=min_ok, flags=pkg.SC_CYCLES_STATUS), _records(f.rt, 80)), "device form, status")):
        _assert_same(got, exp, f"hostile24, min_ok {min_ok}, {what}")
        assert (got[0]["status"] == 0).all() and got[1]["edges"] == 276  # finite is valid, the all-zero record too
        assert (got[0]["max_e2"][f.bad].view(np.uint64) == INF_BITS).all() and (got[0]["max_e2"].view(np.uint64) == INF_BITS).sum() == 3
        assert not np.isnan(got[0]["max_e2"]).any() and not np.isnan(got[0]["min_trace"]).any() and got[0]["min_trace"].min() < -1e100
        assert not got[0]["ok"][f.bad].any()  # +inf is never consistent


def test_one_triangle_of_the_largest_finite_poses(pkg, reg):
    for directions in range(8):
        f = CR.flt_max_triangle(directions)
        cp = _params(pkg, f)
        exp = _expected(pkg, f"FLT_MAX {directions}", f, cp)
        got = reg.pairs_cycles(f.n_sets, f.pairs, f.rt, cp)
        _assert_same(got, exp, f"FLT_MAX, directions {directions:03b}")
        _assert_same(_device(pkg, reg, f.n_sets, f.pairs, cp, _records(f.rt, 48)), exp, f"FLT_MAX, directions {directions:03b}, device form")
        assert (got[1]["triangles"], got[1]["consistent"], got[1]["alive"]) == (1, 0, 0) and np.isfinite(got[0]["min_trace"]).all()
        assert ((got[0]["max_e2"].view(np.uint64) == INF_BITS).all() if directions & 1 else np.isfinite(got[0]["max_e2"]).all()), directions
    patterns = {((1, 0), (2, 1), (0, 2)): True, ((0, 1), (1, 2), (0, 2)): False, ((1, 0), (1, 2), (2, 0)): True}  # -> max_e2 is +inf
    for pairs, inf in patterns.items():
        got = reg.pairs_cycles(3, np.array(pairs), f.rt, cp)
        assert got[0]["max_e2"].view(np.uint64).tolist() == ([INF_BITS] * 3 if inf else [np.float64(3.7726176150972445e+233).view(np.uint64)] * 3)
