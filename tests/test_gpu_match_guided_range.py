"""GPU: the guided matchers — sc_match_guided, sc_match_guided_batch / _pairs and sc_match_guided_poses — at the ends of the fp32 range.

The gate test is `resid2(...) < gate2`, a float `<` applied 32 cells a thread whose outcome decides whether a whole tile's
descriptors are loaded at all, and the finish launch of the poses matcher takes a minimum over residuals of which some may be inf or
NaN.  tests/test_gpu_match_guided*.py run them on points in the unit cube.  Here the points, the poses' translations and the gate
are multiplied by 2^k for k from -70 to 70 (outside test_range_oracle.WIN_C2 the residuals underflow to 0 and subnormals or overflow to
inf), moved 2^20 / 2^22 from the origin (quantised: exact ties in g2, and residuals equal to gate^2), planted with rows at +-3e38, and
the gate is the smallest subnormal (gate^2 = 0), FLT_MAX (gate^2 = +inf: the plain matcher's result) or one step either side of a
planted pair's residual at 2^-56 and 2^62.  The shape is (130, 129), D = 33: two row blocks, three column tiles and a short last
chunk, the smallest at which tile skipping, slices and the look-back are all live; the descriptors stay at unit scale
(tests/test_gpu_match.py::test_magnitudes owns their range).

tests/test_pose_range_ref.py owns the cases and asserts on the references alone (tests/match_guided_ref.py, match_guided_batch_ref.py,
match_guided_poses_ref.py) that they are what they are used for.  Every comparison is bit for bit, in every mode of
match_guided_ref.MODES, through the device forms: corr, the bits of d2 and g2, labels, counts, the flag (never set: every input is
finite) and nothing written behind the count.  The host form runs on one case per matcher.
"""
import numpy as np
import pytest

import match_guided_batch_ref as GB
import match_guided_poses_ref as MP
import match_guided_ref as MG
import test_pose_range_ref as P
from test_gpu_match_guided import _device as _single_device
from test_gpu_match_guided_pairs import _run_pairs
from test_gpu_match_guided_poses import _device as _poses_device
from test_gpu_match_guided_poses import _same as _same_poses

pytestmark = pytest.mark.gpu

MODES = MG.MODES
STATUS = 1  # SC_GUIDE_POSE_STATUS


@pytest.fixture(scope="module")
def greg(pkg):
    r = pkg.Registrar(0)
    yield r
    r.close()


def _same(got, exp, tag):
    (cnt, corr, d2, g2), (exp_c, exp_d, exp_g) = got, exp
    print(tag, "count", cnt, "expected", len(exp_c))
    assert cnt == (len(exp_c), 0), tag                                  # the count, and no flag
    assert np.array_equal(corr, exp_c), tag
    assert d2.view(np.uint32).tobytes() == exp_d.view(np.uint32).tobytes(), tag
    assert g2.view(np.uint32).tobytes() == exp_g.view(np.uint32).tobytes(), tag


# ---- 1: sc_match_guided ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.GUIDED_CASES)
def test_the_single_pose_matcher_equals_the_restatement(pkg, greg, name):
    sc, gate = P.guided_case(name)
    prob = P.guided_problem(name)
    for kw in MODES:
        _same(_single_device(pkg, greg, sc, gate, **kw), prob.match(**kw), (name, kw))
    if name in ("gate:max", "e:max"):                                   # gate^2 = +inf
        for kw in MODES:
            cnt, corr, d2, g2 = _single_device(pkg, greg, sc, gate, **kw)
            if name == "gate:max":                                      # every residual is finite: the plain matcher on the same descriptors
                plain = greg.match(sc.fsrc, sc.ftgt, **kw)
                assert cnt == (plain["n"], 0) and corr.tobytes() == plain["corr"].tobytes() and d2.tobytes() == plain["d2"].tobytes(), kw
            else:                                                       # the inf cells stay out
                assert np.isfinite(g2).all() and not np.isin(corr[:, 0], [10, 70]).any() and not np.isin(corr[:, 1], [11, 70, 90]).any(), kw
    if name == "gate:sub":                                              # gate^2 = 0: nothing, and that is no error
        assert all(_single_device(pkg, greg, sc, gate, **kw)[0] == (0, 0) for kw in MODES)
    if name == "scaled:62":                                             # the host form, both layouts
        for kw in MODES:
            exp = prob.match(**kw)
            for layout in (0, pkg.SC_SOA):
                sp, tp = (sc.src_pts, sc.tgt_pts) if layout == 0 else (np.ascontiguousarray(sc.src_pts.T), np.ascontiguousarray(sc.tgt_pts.T))
                host = greg.match_guided(sp, sc.fsrc, tp, sc.ftgt, sc.Rt, gate=gate, layout=layout, **kw)
                _same(((host["n"], 0), host["corr"], host["d2"], host["g2"]), exp, (name, "host", layout, kw))


@pytest.mark.parametrize("k", P.B_KS)
def test_the_scaled_boundary_of_the_gate(pkg, greg, k):
    """one step of the coordinate either side of the gate, and on it: only the pair inside is admissible, on every matcher"""
    sc, gate = P.boundary_case(k)
    with np.errstate(all="ignore"):
        prob = MG.Problem(*sc.args(), gate)
    assert prob.adm.tolist() == [[False, True, False]]
    for kw in MODES:
        got = _single_device(pkg, greg, sc, gate, **kw)
        _same(got, prob.match(**kw), ("boundary", k, kw))
        assert got[1].tolist() == [[0, 1]], (k, kw)                     # (the nearer descriptors sit at the inadmissible targets)
        # the poses matcher: the admitting record is the second of two
        poses = np.stack([P.scaled_t(MP.shift([0, 80.0, 0]), k), sc.Rt])
        mp = MP.Problem(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, poses, gate)
        dev = _poses_device(pkg, greg, sc, gate, pose=poses, **kw)
        assert dev["flag"] == 0
        _same_poses(dev, mp.match(**kw), ("boundary, poses", k, kw))
        assert dev["corr"].tolist() == [[0, 1]] and dev["label"].tolist() == [1], (k, kw)
    # the batch entry: the problem four times, its targets in four orders
    scenes = [MG.Scene(sc.src_pts, sc.fsrc, np.ascontiguousarray(sc.tgt_pts[o]), np.ascontiguousarray(sc.ftgt[o]), sc.Rt) for o in ([0, 1, 2], [2, 1, 0], [1, 0, 2], [2, 0, 1])]
    batch = GB.Batch(scenes)
    for kw in MODES:
        with np.errstate(all="ignore"):
            exp = GB.match_batch(batch, gate, **kw)
        GB.same(GB.run_device(pkg, greg, batch, gate, **kw), exp, ("boundary, batch", k, kw))
        assert exp[3].tolist() == [[1, 0]] * 4 and exp[0][::kw.get("knn", 1), 1].tolist() == [1, 1, 0, 2], (k, kw)


# ---- 2: sc_match_guided_batch and sc_match_guided_pairs --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.GUIDED_CASES)
def test_the_batch_and_pairs_matchers_equal_the_restatement(pkg, greg, name):
    batch, gate = P.guided_batch(name)
    tab, tgate = P.guided_table(name)
    eb = GB.expand(tab, P.PAIR_LIST, tab["poses"])
    so, to = batch.offsets()
    for kw in MODES:
        knn = kw.get("knn", 1)
        with np.errstate(all="ignore"):
            exp, pexp = GB.match_batch(batch, gate, **kw), GB.match_batch(eb, tgate, **kw)
        got = GB.run_device(pkg, greg, batch, gate, **kw)
        GB.same(got, exp, (name, "batch", kw))
        pgot = _run_pairs(pkg, greg, tab, P.PAIR_LIST, tab["poses"], tgate, **kw)
        GB.same(pgot, pexp, (name, "pairs", kw))
        assert not got[3][:, 1].any() and not pgot[3][:, 1].any()       # finite inputs: no flag
        if name == "gate:sub":
            assert not got[3].any() and not pgot[3].any()
        if name == "gate:max":                                          # the plain matchers on the same descriptors
            sp, fs, tp, ft = batch.packed()
            corr, d2, count = greg.match_batch_raw(fs, so, ft, to, pkg.api.make_match_params(fs.shape[1], **kw))
            pcorr, pd2, pcount, slot = greg.match_pairs(tab["feat"], tab["set_off"], P.PAIR_LIST, **kw)
            assert np.array_equal(count, got[3]) and np.array_equal(pcount, pgot[3]), kw
            for b in range(len(batch)):
                lo, n = int(so[b]) * knn, int(count[b, 0])
                assert corr[lo: lo + n].tobytes() == got[0][lo: lo + n].tobytes() and d2[lo: lo + n].tobytes() == got[1][lo: lo + n].tobytes(), (kw, b)
            for p in range(len(P.PAIR_LIST)):
                lo, n = int(slot[p]), int(pcount[p, 0])
                assert pcorr[lo: lo + n].tobytes() == pgot[0][lo: lo + n].tobytes() and pd2[lo: lo + n].tobytes() == pgot[1][lo: lo + n].tobytes(), (kw, p)
    if name == "scaled:-56":                                            # the host forms, both layouts
        for layout in (0, pkg.SC_SOA):
            for kw in (dict(knn=4), dict(knn=1, mutual=True)):
                with np.errstate(all="ignore"):
                    exp, pexp = GB.match_batch(batch, gate, **kw), GB.match_batch(eb, tgate, **kw)
                GB.same(GB.run_host(greg, batch, gate, layout=layout, **kw), exp, (name, "batch host", layout, kw))
                pts = tab["pts"] if layout == 0 else np.ascontiguousarray(tab["pts"].T)
                corr, d2, g2, count, slot = greg.match_guided_pairs(pts, tab["feat"], tab["set_off"], P.PAIR_LIST, tab["poses"], gate=tgate, layout=layout, **kw)
                assert np.array_equal(count, pexp[3]), (layout, kw)
                for p in range(len(P.PAIR_LIST)):
                    lo, n = int(slot[p]), int(count[p, 0])
                    for a, e in ((corr, pexp[0]), (d2, pexp[1]), (g2, pexp[2])):
                        assert a[lo: lo + n].tobytes() == e[lo: lo + n].tobytes(), (layout, kw, p)


# ---- 3: sc_match_guided_poses ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", P.POSES_KS)
@pytest.mark.parametrize("name,k", P.POSES_CASES)
def test_the_poses_matcher_equals_the_restatement(pkg, greg, name, k, K):
    sc, poses, status, gate = P.poses_case(name, K, k)
    prob = P.poses_problem(name, K, k)
    pose, flags = (poses, 0) if status is None else (MP.records(poses, status), STATUS)
    for kw in MODES:
        exp = prob.match(**kw)
        dev = _poses_device(pkg, greg, sc, gate, pose=pose, flags=flags, **kw)
        assert dev["flag"] == 0, (name, k, K, kw)
        _same_poses(dev, exp, (name, k, K, kw))
        if name == "allhost":
            assert dev["n"] == 0
        elif name == "hostile":                                         # the ordinary record's label and residual, bit for bit the single-pose entry's
            one = _single_device(pkg, greg, sc, gate, **kw)
            assert (dev["label"] == 1).all() and dev["n"] == one[0][0] > 0 and dev["g2"].tobytes() == one[3].tobytes(), (k, K, kw)
        elif name == "off":
            assert (dev["label"] == 1).all() and dev["n"] > 0
    if K == 5:                                                          # the host form
        for kw in MODES:
            host = greg.match_guided_poses(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, pose, gate=gate, flags=flags, **kw)
            _same_poses(host, prob.match(**kw), (name, k, K, "host", kw))


@pytest.mark.parametrize("name", ["scaled:-70", "scaled:-56", "scaled:62", "scaled:70", "translated:20:22", "e", "e:max", "gate:sub", "gate:max"])
def test_the_poses_matcher_with_one_record_is_the_single_pose_matcher(pkg, greg, name):
    """K = 1, and K = 3 with two far records around the scene's: the cases of section 1 through the poses matcher's own gate loop and
    finish launch"""
    sc, gate = P.guided_case(name)
    prob = P.guided_problem(name)
    k = int(name.split(":")[1]) if name.startswith("scaled") else 0
    far = [P.scaled_t(MP.shift([0, 80.0 + i, 0]), k) for i in range(2)]
    for poses, label in ((sc.Rt[None, :], 0), (np.stack([far[0], sc.Rt, far[1]]), 1)):
        with np.errstate(all="ignore"):
            mp = MP.Problem(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, poses, gate)
        for kw in MODES:
            exp = mp.match(**kw)
            dev = _poses_device(pkg, greg, sc, gate, pose=poses, **kw)
            assert dev["flag"] == 0, (name, kw)
            _same_poses(dev, exp, (name, len(poses), kw))
            if name not in ("translated:20:22", "e:max", "gate:max"):   # (there the far records admit cells as well)
                c, d, g = prob.match(**kw)
                assert np.array_equal(dev["corr"], c) and dev["g2"].tobytes() == g.tobytes() and (dev["label"] == label).all(), (name, kw)
