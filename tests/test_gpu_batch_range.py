"""GPU: sc_register_batch and its slot form (sc_register_batch_features) at the ends of the fp32 range, and the cut among equal keys
at every boundary of its three find_cut passes.

sc_batch.hip restates the whole of sc_register in its own shape — stage A as a wave ballot, edge weights recomputed per key, Kabsch
and scoring fused, a two-word winner — and promises the record sc_register returns for the problem alone.  tests/test_gpu_batch.py
checks that at unit scale; here the inputs are those of tests/test_gpu_range.py on the batch scenes.  tests/test_batch_range_ref.py
owns them and asserts, on the reference alone, that they are what they are used for and that no problem exceeds batch_ref.TRI_CAP.

The expected value is tests/batch_ref.py (problem b alone through the CPU restatement), every record field and mask byte, bit for
bit; an SC_OK problem is also compared with sc_register on it alone.  Every case runs alone and packed with the other cases of its
parameter set (a launch has one sc_params) in both layouts; all magnitudes also share ONE launch under the unit parameters.
"""
import numpy as np
import pytest

import batch_ref
import match_batch_ref as M
import test_batch_range_ref as R
from conftest import nan_equal_bits
from test_gpu_batch import FIELDS, SC_FLAG_EXACT_TOTAL, _assert_batch, _run
from test_gpu_match_batch import _assert_features
from test_range_oracle import UNIT, pow2

pytestmark = pytest.mark.gpu

SC_OK, SC_ENOHYP = batch_ref.SC_OK, batch_ref.SC_ENOHYP


def _exp(pkg, O, names, mode=0):
    refs = [R.case_ref(pkg, O, name, mode) for name in names]
    recs = np.zeros(len(refs), batch_ref.RESULT_DTYPE)
    for b, r in enumerate(refs):
        recs[b] = r[3]
    assert int(recs["tri_total"].max()) <= batch_ref.TRI_CAP
    return [(r[0], r[1]) for r in refs], (recs, [r[4] for r in refs])


def _assert_solo(pkg, reg, problem, kw, rec, mask, what, **extra):
    """the record against sc_register on the problem alone"""
    s, t = problem
    solo = reg.register(s, t, params=pkg.make_params(**kw, flags=SC_FLAG_EXACT_TOTAL, **extra))
    st = solo["stats"]
    assert [int(rec[f]) for f in FIELDS] == [solo["status"], len(s), st["edges"], st["tri_kept"], st["tri_total"], st["best_rank"], st["best_count"]], what
    assert nan_equal_bits(rec["Rt"], np.concatenate([solo["R"].ravel(), solo["t"]])), what
    assert np.array_equal(mask, solo["mask"]), what


# ---- 1: every family, alone and packed by parameter set, both layouts ---------------------------------------------------------
_GPU = {}  # name -> (record, mask) of the GPU, for the metamorphic check


GROUPS = {"+".join(names) if len(names) < 4 else f"{names[0]}+{len(names) - 1}": (kw, names) for kw, names in R.groups()}


@pytest.mark.parametrize("gid", list(GROUPS))
def test_every_family_equals_the_reference_and_sc_register(pkg, O, reg, gid):
    kw, names = GROUPS[gid]
    problems, exp = _exp(pkg, O, names)
    got = _run(reg, pkg, problems, kw)
    _assert_batch(got, exp, f"{gid} AoS")
    _assert_batch(_run(reg, pkg, problems, kw, soa=True), exp, f"{gid} SoA")
    recs, mask, off = got
    for b, name in enumerate(names):
        _GPU[name] = (recs[b].copy(), mask[off[b]: off[b + 1]].copy())
        if len(names) > 1:                                                # ... and alone: the same bytes
            solo = _run(reg, pkg, [problems[b]], kw)
            assert solo[0][0].tobytes() == recs[b].tobytes() and np.array_equal(solo[1], _GPU[name][1]), name
            _assert_batch(_run(reg, pkg, [problems[b]], kw, soa=True), (exp[0][b: b + 1], exp[1][b: b + 1]), f"{name} alone, SoA")
        if int(recs[b]["status"]) == SC_OK:
            _assert_solo(pkg, reg, problems[b], kw, recs[b], _GPU[name][1], name)


def test_all_magnitudes_in_one_launch(pkg, O, reg):
    """Workgroups side by side at 2^-70 .. 2^70, 2^24 from the origin and at +-3e38, under the unit parameters."""
    problems = R.one_launch_problems(pkg)
    kw = dict(UNIT, max_triangles=R.T)
    exp = R.one_launch_ref(pkg, O)
    assert len(problems) <= 40
    _assert_batch(_run(reg, pkg, problems, kw), exp, "one launch AoS")
    _assert_batch(_run(reg, pkg, problems, kw, soa=True), exp, "one launch SoA")


@pytest.mark.parametrize("n", list(R.SCENES))
def test_inside_the_window_the_gpu_equals_itself_at_unit_scale(pkg, O, reg, n):
    """Without the oracle: the record at k is the record at k = 0 with t times 2^k (tests/test_batch_range_ref.py: the
    reference is covariant on these scenes at these k)."""
    def gpu(k):
        name = f"a:{n}:{k}"
        if name not in _GPU:
            s, t, kw = R.case_input(pkg, name)
            recs, mask, _ = _run(reg, pkg, [(s, t)], kw)
            _GPU[name] = (recs[0].copy(), mask.copy())
        return _GPU[name]
    r0, m0 = gpu(0)
    assert int(r0["status"]) == SC_OK
    ks = R.metamorphic_ks()
    assert len(ks) >= 3
    for k in ks:
        r, m = gpu(k)
        assert [int(r[f]) for f in FIELDS] == [int(r0[f]) for f in FIELDS], (n, k)
        assert np.array_equal(m, m0), (n, k)
        assert r["Rt"][:9].tobytes() == r0["Rt"][:9].tobytes() and r["Rt"][9:].tobytes() == (r0["Rt"][9:] * pow2(k)).tobytes(), (n, k)


# ---- 2: the truncated score modes where 1 / tau^2 and 1 / tau are inf, 0 or tiny ----------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["f:tau-30", "f:tau25", "a:300:-56", "a:300:62"])
def test_score_modes(pkg, O, reg, name, mode):
    problems, exp = _exp(pkg, O, [name], mode)
    kw = R.case_kw(name)
    got = _run(reg, pkg, problems, kw, score_mode=mode)
    _assert_batch(got, exp, f"{name} mode {mode}")
    _assert_batch(_run(reg, pkg, problems, kw, soa=True, score_mode=mode), exp, f"{name} mode {mode} SoA")
    if int(got[0][0]["status"]) == SC_OK:
        _assert_solo(pkg, reg, problems[0], kw, got[0][0], got[1], f"{name} mode {mode}", score_mode=mode)


# ---- 3: the cut among equal keys --------------------------------------------------------------------------------------------------
_CUT_REF = {}


@pytest.mark.parametrize("rank_mode", [0, 1])
@pytest.mark.parametrize("what", list(R.CUTS))
def test_the_cut_among_equal_keys(pkg, O, reg, what, rank_mode):
    """exact100: 161 700 equal keys, two words a row, 7 column chunks.  T puts the last kept triangle where `what` says: the k, the
    j or the row at or across bit 63 | 64, the last / first triangle of a row or an edge (find_cut's need == pre + v0 and rem == 1),
    a j at a chunk edge.  (Every hypothesis is the same translation here: the winner is (0, 1, 2) wherever the cut falls — this test
    says that the three passes end and leave a cut that keeps it; the next test makes the cut itself visible.)"""
    problem = R.exact100()
    kw = dict(UNIT, max_triangles=R.CUTS[what], rank_mode=rank_mode)
    if (what, rank_mode) not in _CUT_REF:
        _CUT_REF[what, rank_mode] = batch_ref.batch(O, [problem], kw)
    exp = _CUT_REF[what, rank_mode]
    assert int(exp[0][0]["tri_total"]) == R.EXACT_TOTAL <= batch_ref.TRI_CAP
    assert int(exp[0][0]["tri_kept"]) == min(R.CUTS[what], R.EXACT_TOTAL)
    _assert_batch(_run(reg, pkg, [problem], kw), exp, f"{what} rank_mode {rank_mode}")


@pytest.mark.parametrize("what", list(R.CUT_TRIANGLES))
def test_the_triangle_at_the_cut_wins_when_it_is_kept(pkg, O, reg, what):
    """The same cuts made visible (tests/test_batch_range_ref.py, cut_scene): the triangle at the cut is the only good hypothesis
    among the first T, so T and T - 1 differ in best_rank, best_count, (R, t) and the mask."""
    problem, nh, T, at, before = R.cut_scene_ref(O, what)
    assert int(at[0][0]["best_count"]) == nh > int(before[0][0]["best_count"])
    _assert_batch(_run(reg, pkg, [problem], dict(R.CUT_KW, max_triangles=T)), at, f"{what} T={T}")
    _assert_batch(_run(reg, pkg, [problem], dict(R.CUT_KW, max_triangles=T - 1)), before, f"{what} T={T - 1}")


# ---- 4: the slot kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-64, 30, 64])
def test_the_slot_kernel_on_an_identity_match(pkg, O, reg, k):
    """batch_register_kernel<BatchSlotJob> takes n and the flag from device words.  Descriptors that are the rows of the identity
    match every point to itself (mutual, knn 1), so the matched points are the a:192 points in their order, and the records are
    those of the plain form."""
    name = f"a:192:{k}"
    s, t, kw, rec, mask = R.case_ref(pkg, O, name)
    eye = np.eye(len(s), dtype=np.float32)
    mkw = dict(knn=1, mutual=True)
    with np.errstate(over="ignore", under="ignore"):
        exp = M.features_one(O, s, eye, t, eye, mkw, kw)
    assert exp["n"] == len(s) and np.array_equal(exp["corr"][:, 0], np.arange(len(s))) and np.array_equal(exp["corr"][:, 1], np.arange(len(s)))
    assert exp["rec"].tobytes() == rec.tobytes() and np.array_equal(exp["mask"], mask)      # the composition IS the plain case
    plain = _run(reg, pkg, [(s, t)], kw)
    _assert_batch(plain, (np.array([rec]), [mask]), f"{name} plain")
    for layout in (pkg.SC_AOS, pkg.SC_SOA):
        out = reg.register_batch_features([(s, eye, t, eye)], params=pkg.make_params(**kw, layout=layout), **mkw)
        _assert_features(out, [exp], f"{name} slot form, layout {layout}")
        o = out[0]
        assert [o["status"]] + [o["stats"][f] for f in FIELDS[1:]] == [int(plain[0][0][f]) for f in FIELDS], name
        assert np.concatenate([o["R"].ravel(), o["t"]]).tobytes() == plain[0][0]["Rt"].tobytes() and np.array_equal(o["mask"], plain[1]), name
