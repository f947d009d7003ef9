"""GPU: sc_polish_batch, its slot form and its pairs form at the ends of the fp32 range, and on input poses that are caller data.

polish_batch_kernel (sc_polish_batch.hip) shares the refit iteration with sc_polish, but the score of the input pose and of the last
iterate in the three score modes, the finiteness gates on the pose, the mask, the pass-through rules and the staging are its own, and
tests/test_gpu_polish_batch.py runs them on unit-scale scenes from the batch winner only.  Here the inputs are those of
tests/test_gpu_batch_range.py, and the table of shifted and hostile poses of tests/test_batch_tail_range_ref.py, which owns the
cases and asserts on the reference alone that they stop in every way, at every scale.

The expected value is tests/polish_batch_ref.py: every field of every record, Rt through nan_equal_bits, every mask byte.  No
tolerances.  A case runs packed with the other cases of its launch (one sc_params, one max_iter) and alone, in both layouts; a
winner's polish with SC_OK is also compared with sc_register + sc_polish(candidates = 1) on the problem alone (sc_refit.hpp's promise).
"""
from itertools import zip_longest

import numpy as np
import pytest

import batch_ref
import polish_batch_ref as PB
import test_batch_range_ref as R
import test_batch_tail_range_ref as TR
from conftest import nan_equal_bits
from test_gpu_batch import SC_FLAG_EXACT_TOTAL
from test_gpu_pairs import run_packed, run_pairs
from test_gpu_polish_batch import _assert_polish, _both, _layout, _pack
from test_range_oracle import UNIT, pow2

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = batch_ref.SC_OK, batch_ref.SC_EINVAL, batch_ref.SC_ENOHYP
MAX_ITER = TR.MAX_ITER

_GPU = {}  # (name, pose) -> (record, mask) of the GPU at max_iter 16, for the metamorphic check


def _cases(pkg, O, cases, mode=0):
    """cases: (name, pose, max_iter) -> (problems, input records, expected (records, masks))"""
    refs = [TR.polish_case(pkg, O, name, pose, mi, mode) for name, pose, mi in cases]
    rin = np.array([r[3] for r in refs], batch_ref.RESULT_DTYPE)
    exp = np.array([r[4][0] for r in refs], PB.RESULT_DTYPE)
    return [(r[0], r[1]) for r in refs], rin, (exp, [r[4][1] for r in refs])


def _polish(reg, pkg, problems, kw, mode, max_iter, soa, recs):
    """sc_polish_batch alone on hand-given records -> (polish records, mask, offset)"""
    src, tgt, off = _pack(problems)
    src, tgt = _layout(pkg, src, tgt, soa)
    p = pkg.make_params(**kw, score_mode=mode, layout=pkg.SC_SOA if soa else pkg.SC_AOS)
    pol, pmask = reg.polish_batch_raw(src, tgt, off, p, pkg.make_polish_params(candidates=1, max_iter=max_iter), recs)
    return pol, pmask, off


def _assert_solo(pkg, reg, problem, kw, mode, max_iter, pol, mask, what):
    """the record against sc_register then sc_polish(candidates = 1) on the problem alone"""
    s, t = problem
    solo = reg.register(s, t, params=pkg.make_params(**kw, score_mode=mode, flags=SC_FLAG_EXACT_TOTAL))
    assert solo["status"] == SC_OK, what
    one = reg.polish(candidates=1, max_iter=max_iter)
    k = one["cand"][0]
    assert one["status"] == SC_OK and one["n_cand"] == 1, what
    assert nan_equal_bits(pol["Rt"], np.concatenate([one["R"].ravel(), one["t"]])) and nan_equal_bits(pol["Rt"], k["Rt"]), what
    assert np.array_equal(mask, one["mask"]), what
    assert (int(pol["score0"]), int(pol["score"]), int(pol["iters"])) == (int(k["score0"]), int(k["score"]), int(k["iters"])), what


def _check_launch(pkg, O, reg, kw, max_iter, cases, mode, what, solo=True):
    """packed and alone, both layouts, against the reference; the winners' polishes also against the single-problem path"""
    problems, rin, exp = _cases(pkg, O, cases, mode)
    assert len(problems) <= 40
    for soa in (False, True):
        _, pol, pmask, off = _both(reg, pkg, problems, kw, mode, max_iter, soa, recs=rin)
        _assert_polish(pol, pmask, off, exp, f"{what} soa={soa}")
        for b, case in enumerate(cases):
            if len(cases) > 1:  # ... and alone: the same bytes
                apol, amask, _ = _polish(reg, pkg, [problems[b]], kw, mode, max_iter, soa, rin[b: b + 1])
                assert apol[0].tobytes() == pol[b].tobytes() and np.array_equal(amask, pmask[off[b]: off[b + 1]]), (what, case, soa)
    for b, (name, pose, mi) in enumerate(cases):
        if mi == MAX_ITER and mode == 0:
            _GPU[name, pose] = (pol[b].copy(), pmask[off[b]: off[b + 1]].copy())
        if solo and pose == "winner" and int(rin[b]["status"]) == SC_OK:
            _assert_solo(pkg, reg, problems[b], kw, mode, mi, pol[b], pmask[off[b]: off[b + 1]], f"{what} {name}")


def _chunks(groups, size=40):
    out = {}
    for kw, mi, cases in groups:
        for lo in range(0, len(cases), size):
            part = cases[lo: lo + size]
            gid = f"{part[0][0]}/{part[0][1]}/{mi}" + (f"+{len(part) - 1}" if len(part) > 1 else "")
            out[gid] = (kw, mi, part)
    return out


# ---- 1: every name from the winner's pose, packed by parameter set and alone, both layouts -----------------------------------------
WINNERS = _chunks(TR.polish_groups([(name, "winner", MAX_ITER) for name in R.NAMES]))


@pytest.mark.parametrize("gid", list(WINNERS))
def test_the_winners_polish_equals_the_reference_and_sc_polish(pkg, O, reg, gid):
    kw, mi, cases = WINNERS[gid]
    _check_launch(pkg, O, reg, kw, mi, cases, 0, gid)


# ---- 2: the table of shifted and hostile poses ----------------------------------------------------------------------------------------
TABLE = _chunks(TR.polish_groups(TR.POSES))


@pytest.mark.parametrize("gid", list(TABLE))
def test_the_pose_table_equals_the_reference(pkg, O, reg, gid):
    kw, mi, cases = TABLE[gid]
    _check_launch(pkg, O, reg, kw, mi, cases, 0, gid)


@pytest.mark.parametrize("k", [0, -64, 64])
def test_hostile_and_shifted_poses_between_good_problems(pkg, O, reg, k):
    """[good, bad, good, bad, ...] in one launch: a flagged or declined problem leaves its neighbours' records and mask bytes what a
    launch of the good ones alone gives, and its own mask bytes zero."""
    good = [(f"a:{n}:{k}", "winner", MAX_ITER) for n in R.SCENES] + [(f"a:300:{k}", "shift:0.5", MAX_ITER)]
    if k == 0:
        good += [("e", "winner", MAX_ITER), ("b:far62", "winner", MAX_ITER)]
    bad = [(name, h, MAX_ITER) for name in ((f"a:300:{k}", "e") if k == 0 else (f"a:300:{k}",)) for h in TR.HOSTILE] + [(f"a:300:{k}", "shift:3.0", MAX_ITER)]
    order = [c for pair in zip_longest(bad, good[:-1]) for c in pair if c is not None] + good[-1:]   # bad first, good last
    assert sorted(order) == sorted(good + bad) and order[0] in bad and order[1] in good
    kw = TR.tail_kw(good[0][0])
    assert all(np.float32(TR.tail_kw(c[0])[x]) == np.float32(kw[x]) for c in order for x in kw)   # one sc_params (its lengths are fp32)
    problems, rin, exp = _cases(pkg, O, order)
    gproblems, grin, gexp = _cases(pkg, O, good)
    for soa in (False, True):
        pol, pmask, off = _polish(reg, pkg, problems, kw, 0, MAX_ITER, soa, rin)
        _assert_polish(pol, pmask, off, exp, f"k={k} soa={soa}")
        gpol, gmask, goff = _polish(reg, pkg, gproblems, kw, 0, MAX_ITER, soa, grin)
        _assert_polish(gpol, gmask, goff, gexp, f"k={k} the good ones, soa={soa}")
        for pos, case in enumerate(good):
            b = order.index(case)
            assert pol[b].tobytes() == gpol[pos].tobytes() and int(pol[b]["status"]) == SC_OK and int(pol[b]["score"]) > 3, (k, case)
            assert np.array_equal(pmask[off[b]: off[b + 1]], gmask[goff[pos]: goff[pos + 1]]) and pmask[off[b]: off[b + 1]].any(), (k, case)
        for case in bad:
            b = order.index(case)
            assert int(pol[b]["status"]) in (SC_OK, SC_EINVAL, SC_ENOHYP) and int(pol[b]["stop"]) == PB.STOP_DECLINED and int(pol[b]["iters"]) == 0, (k, case)
            assert not pmask[off[b]: off[b + 1]].any(), (k, case)
            want = batch_ref.IDENT if int(pol[b]["status"]) != SC_OK else rin[b]["Rt"]
            assert pol[b]["Rt"].tobytes() == want.tobytes(), (k, case)      # flagged: the identity; declined: the input pose's bits


# ---- 3: all magnitudes in one launch -----------------------------------------------------------------------------------------------
def test_all_magnitudes_in_one_launch(pkg, O, reg):
    """Workgroups side by side at 2^-70 .. 2^70, 2^24 from the origin and at +-3e38, under the unit parameters."""
    problems, rin, exp = TR.polish_one_launch(pkg, O)
    kw = dict(UNIT, max_triangles=R.T)
    assert len(problems) <= 40
    for soa in (False, True):
        r, pol, pmask, off = _both(reg, pkg, problems, kw, 0, MAX_ITER, soa)   # from the GPU's own batch records
        assert list(r["status"]) == list(rin["status"]) and all(nan_equal_bits(a["Rt"], b["Rt"]) for a, b in zip(r, rin))
        _assert_polish(pol, pmask, off, exp, f"one launch soa={soa}")


# ---- 4: inside the window the GPU equals itself at unit scale -------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(R.SCENES))
def test_inside_the_window_the_gpu_equals_itself_at_unit_scale(pkg, O, reg, n):
    """Without the oracle's values: the polish record at k is the one at k = 0 with t times 2^k, from the winner's pose and from the
    shifted ones (tests/test_batch_tail_range_ref.py: the reference is covariant on these scenes at these k)."""
    def gpu(k, pose):
        name = f"a:{n}:{k}"
        if (name, pose) not in _GPU:
            problems, rin, _ = _cases(pkg, O, [(name, pose, MAX_ITER)])
            pol, pmask, _ = _polish(reg, pkg, problems, TR.tail_kw(name), 0, MAX_ITER, False, rin)
            _GPU[name, pose] = (pol[0].copy(), pmask.copy())
        return _GPU[name, pose]
    ks = R.metamorphic_ks()
    assert len(ks) >= 3
    for pose in ("winner", "shift:0.5", "shift:1.5"):
        r0, m0 = gpu(0, pose)
        assert int(r0["status"]) == SC_OK
        for k in ks:
            r, m = gpu(k, pose)
            assert [int(r[f]) for f in PB.FIELDS] == [int(r0[f]) for f in PB.FIELDS] and np.array_equal(m, m0), (n, k, pose)
            assert r["Rt"][:9].tobytes() == r0["Rt"][:9].tobytes() and r["Rt"][9:].tobytes() == (r0["Rt"][9:] * pow2(k)).tobytes(), (n, k, pose)


# ---- 5: the truncated score modes where 1 / tau^2 and 1 / tau are inf, 0 or tiny --------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", TR.MODE_NAMES)
def test_score_modes(pkg, O, reg, name, mode):
    cases = [(name, pose, MAX_ITER) for pose in TR.MODE_POSES]
    _check_launch(pkg, O, reg, TR.tail_kw(name), MAX_ITER, cases, mode, f"{name} mode {mode}")


# ---- 6: the slot form and the pairs form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-64, 30, 64])
def test_the_slot_and_pairs_forms_on_an_identity_match(pkg, O, reg, k):
    """polish_batch_kernel<PolishBatchSlotJob> and <PolishBatchPairsJob> gather the problem through corr and take n from a device
    word.  Descriptors that are the rows of the identity match every point to itself (mutual, knn 1), so the gathered problem is
    a:192:k in its order, and the record and the mask are the plain form's."""
    name = f"a:192:{k}"
    s, t, kw, rin, (erec, emask) = TR.polish_case(pkg, O, name)
    n = len(s)
    eye = np.eye(n, dtype=np.float32)
    tab = dict(sets=[(s, eye), (t, eye)], pts=np.concatenate([s, t]), feat=np.concatenate([eye, eye]), set_off=np.array([0, n, 2 * n], np.uint32))
    pairs = np.array([(0, 1)], np.uint32)
    mp = pkg.api.make_match_params(n, knn=1, mutual=True)
    q = pkg.make_polish_params(candidates=1, max_iter=MAX_ITER)
    plain, plain_mask, off = _polish(reg, pkg, [(s, t)], kw, 0, MAX_ITER, False, np.array([rin], batch_ref.RESULT_DTYPE))
    _assert_polish(plain, plain_mask, off, (np.array([erec]), [emask]), f"{name} plain")
    assert int(plain[0]["status"]) == SC_OK and int(plain[0]["iters"]) >= 1
    for layout in (pkg.SC_AOS, pkg.SC_SOA):
        p = pkg.make_params(**kw, layout=layout)
        for form, run in (("slots", run_packed), ("pairs", run_pairs)):
            out = run(reg, pkg, tab, pairs, mp, p, q)
            what = f"{name} {form} layout {layout}"
            assert out["count"][0].tolist() == [n, 0] and np.array_equal(out["corr"][:n], np.stack([np.arange(n)] * 2, 1)), what
            g = out["res"][0]
            assert int(g["status"]) == int(rin["status"]) and nan_equal_bits(g["Rt"], rin["Rt"]), what      # the input pose IS the case's
            print(what, [int(out["pol"][0][f]) for f in PB.FIELDS], "| plain", [int(plain[0][f]) for f in PB.FIELDS])
            assert out["pol"][0].tobytes() == plain[0].tobytes(), what
            assert np.array_equal(out["pmask"][:n], plain_mask), what
