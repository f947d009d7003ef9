"""GPU: sc_register_instances_batch and its features / slot form at the ends of the fp32 range.

The ROUNDS instantiations of batch_register_kernel (sc_batch.hip) score through score_alive — a second copy of the scoring loop, four
correspondences at a time under the alive word —, claim through is_inliers under a wave ballot and stop on min_score against the top
word of a 64-bit key.  tests/test_gpu_instances_batch.py runs them at unit scale, where almost every problem holds exactly two
motions.  Here the scenes are scaled by 2^k, translated to 2^20 .. 2^22 and planted with rows at +-3e38:
tests/test_batch_tail_range_ref.py owns the cases and asserts on the reference alone that the second motion is lost (k = -64), that
every plane is filled (k = 66), that a later winner has a claimed vertex (k = -70), that the rounds end on min_score with a score
left, and that no problem exceeds batch_ref.TRI_CAP.

The expected value is tests/instances_batch_ref.py: every field of every record of every plane, every label, every nfound, bit for
bit.  No tolerances.  A case runs packed with the other cases of its parameter set and alone, in both layouts; an SC_OK problem is
also compared with sc_register_instances on it alone, and plane 0 with sc_register_batch's record.
"""
import numpy as np
import pytest

import batch_ref
import test_batch_tail_range_ref as TR
from conftest import nan_equal_bits
from test_gpu_instances_batch import FIELDS, SC_FLAG_EXACT_TOTAL, _assert_batch, _bytes, _pack, _run
from test_range_oracle import UNIT, pow2

pytestmark = pytest.mark.gpu

SC_OK = batch_ref.SC_OK
K = TR.MAX_INSTANCES

_GPU = {}  # name -> (planes, labels, nfound) of the GPU, for the metamorphic check


def _exp(pkg, O, names, mode=0):
    """-> (problems, (records (K, B), labels, nfound)) of the reference"""
    refs = [TR.inst_ref(pkg, O, name, mode) for name in names]
    recs = np.zeros((K, len(refs)), batch_ref.RESULT_DTYPE)
    for b, r in enumerate(refs):
        recs[:, b] = r[3]
    assert int(recs["tri_total"].max()) <= batch_ref.TRI_CAP
    return [(r[0], r[1]) for r in refs], (recs, [r[4] for r in refs], np.array([r[5] for r in refs], np.uint32))


def _one(exp, b):
    return exp[0][:, b: b + 1], exp[1][b: b + 1], exp[2][b: b + 1]


def _assert_solo(pkg, reg, problem, kw, mode, got, b, what):
    """problem b of `got` against sc_register_instances on it alone"""
    recs, label, nfound, off = got
    s, t = problem
    solo = reg.register_instances(s, t, max_instances=K, min_score=TR.min_score_of(mode),
                                  params=pkg.make_params(**kw, score_mode=mode, flags=SC_FLAG_EXACT_TOTAL))
    k = len(solo["score"])
    assert k == int(nfound[b]) and solo["status"] == int(recs[0, b]["status"]) == SC_OK, what
    assert nan_equal_bits(solo["Rt"], recs[:k, b]["Rt"]) and np.array_equal(solo["score"], recs[:k, b]["best_count"]), what
    assert np.array_equal(solo["label"], label[off[b]: off[b + 1]]), what
    st = solo["stats"]
    assert [int(recs[0, b][f]) for f in FIELDS[1:]] == [len(s), st["edges"], st["tri_kept"], st["tri_total"], st["best_rank"], st["best_count"]], what


def _check_launch(pkg, O, reg, kw, names, mode, what):
    problems, exp = _exp(pkg, O, names, mode)
    ms = TR.min_score_of(mode)
    assert len(problems) <= 40
    got = _run(reg, pkg, problems, kw, K, ms, score_mode=mode)
    _assert_batch(got, exp, f"{what} AoS")
    _assert_batch(_run(reg, pkg, problems, kw, K, ms, soa=True, score_mode=mode), exp, f"{what} SoA")
    # plane 0 is sc_register_batch's record
    src, tgt, off = _pack(problems)
    brecs, _ = reg.register_batch_raw(src, tgt, off, pkg.make_params(**kw, score_mode=mode))
    assert got[0][0].tobytes() == brecs.tobytes(), what
    for b, name in enumerate(names):
        if mode == 0:
            _GPU[name] = _bytes(got, b)
        if len(names) > 1:  # ... and alone: the same bytes
            assert _bytes(_run(reg, pkg, [problems[b]], kw, K, ms, score_mode=mode), 0) == _bytes(got, b), name
            _assert_batch(_run(reg, pkg, [problems[b]], kw, K, ms, soa=True, score_mode=mode), _one(exp, b), f"{name} alone, SoA")
        if int(got[0][0, b]["status"]) == SC_OK:
            _assert_solo(pkg, reg, problems[b], kw, mode, got, b, f"{what} {name}")


# ---- 1: every case, alone and packed by parameter set, both layouts -----------------------------------------------------------------
GROUPS = {"+".join(names): (kw, names) for kw, names in TR.inst_groups()}


@pytest.mark.parametrize("gid", list(GROUPS))
def test_every_case_equals_the_reference_and_sc_register_instances(pkg, O, reg, gid):
    kw, names = GROUPS[gid]
    _check_launch(pkg, O, reg, kw, names, 0, gid)


def test_all_magnitudes_in_one_launch(pkg, O, reg):
    """Workgroups side by side at 2^-70 .. 2^66, 2^22 from the origin and at +-3e38, under the unit parameters."""
    problems, exp = TR.inst_one_launch(pkg, O)
    kw = dict(UNIT, max_triangles=TR.T)
    assert len(problems) <= 40
    _assert_batch(_run(reg, pkg, problems, kw, K, TR.min_score_of(0)), exp, "one launch AoS")
    _assert_batch(_run(reg, pkg, problems, kw, K, TR.min_score_of(0), soa=True), exp, "one launch SoA")


# ---- 2: inside the window the GPU equals itself at unit scale -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [n for n, _ in TR.I_SCENES])
def test_inside_the_window_the_gpu_equals_itself_at_unit_scale(pkg, O, reg, n):
    """Without the oracle: every plane at k is the plane at k = 0 with t times 2^k, the labels and nfound are the same
    (tests/test_batch_tail_range_ref.py: the reference is covariant on these scenes at these k)."""
    def gpu(k):
        name = f"s:{n}:{k}"
        if name not in _GPU:
            s, t, kw = TR.inst_input(pkg, name)
            _GPU[name] = _bytes(_run(reg, pkg, [(s, t)], kw, K, TR.min_score_of(0)), 0)
        planes, label, found = _GPU[name]
        return np.frombuffer(planes, batch_ref.RESULT_DTYPE), label, found
    p0, l0, f0 = gpu(0)
    assert f0 == 2 and int(p0[0]["status"]) == SC_OK
    ks = TR.inst_metamorphic_ks()
    assert len(ks) >= 3
    for k in ks:
        p, l, f = gpu(k)
        assert f == f0 and l == l0, (n, k)
        for a, b in zip(p, p0):
            assert [int(a[x]) for x in FIELDS] == [int(b[x]) for x in FIELDS], (n, k)
            assert a["Rt"][:9].tobytes() == b["Rt"][:9].tobytes() and a["Rt"][9:].tobytes() == (b["Rt"][9:] * pow2(k)).tobytes(), (n, k)


# ---- 3: the truncated score modes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("k", [-56, 62])
def test_score_modes(pkg, O, reg, k, mode):
    names = [f"s:{n}:{k}" for n, _ in TR.I_SCENES]
    assert set(names) <= set(TR.I_MODE_NAMES)
    _check_launch(pkg, O, reg, TR.inst_kw(names[0]), names, mode, f"k={k} mode {mode}")


# ---- 4: the features / slot form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-64, 30, 64])
def test_the_features_form_on_an_identity_match(pkg, O, reg, k):
    """batch_register_kernel<BatchSlotJob, ROUNDS> takes n and the flag from device words and gathers through corr.  Descriptors that
    are the rows of the identity match every point to itself (mutual, knn 1), so the gathered problems are s:128:k and s:257:k in
    their order, and planes, labels and nfound are the plain form's — the reference's."""
    import torch
    names = [f"s:{n}:{k}" for n in (128, 257)]
    problems, exp = _exp(pkg, O, names)
    kw = TR.inst_kw(names[0])
    plain = _run(reg, pkg, problems, kw, K, TR.min_score_of(0))
    _assert_batch(plain, exp, f"k={k} plain")
    dim = 257
    feats = [np.eye(len(s), dim, dtype=np.float32) for s, _ in problems]
    mp = pkg.api.make_match_params(dim, knn=1, mutual=True)
    so = reg._offsets([len(s) for s, _ in problems])
    nb, slots = len(problems), int(so[-1])
    fe = np.concatenate(feats)
    ident = np.concatenate([np.arange(len(s)) for s, _ in problems])
    for layout in (pkg.SC_AOS, pkg.SC_SOA):
        p = pkg.make_params(**kw, layout=layout)
        src, tgt = np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems])
        if layout == pkg.SC_SOA:
            src, tgt = np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)
        d_src, d_tgt, d_fe = (torch.from_numpy(a).cuda() for a in (src, tgt, fe))
        d_res = torch.full((K * nb * 80,), 0xAB, dtype=torch.uint8, device="cuda")
        d_corr = torch.full((slots, 2), -7, dtype=torch.int32, device="cuda"); d_d2 = torch.zeros(slots, dtype=torch.float32, device="cuda")
        d_count = torch.full((nb, 2), 9, dtype=torch.int32, device="cuda")
        d_label = torch.full((slots,), 77, dtype=torch.int32, device="cuda"); d_nfound = torch.full((nb,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        reg.register_instances_batch_features_device(d_src.data_ptr(), d_fe.data_ptr(), so, d_tgt.data_ptr(), d_fe.data_ptr(), so, mp, p, K,
                                                     TR.min_score_of(0), d_res.data_ptr(), d_corr.data_ptr(), d_d2.data_ptr(), d_count.data_ptr(),
                                                     d_label.data_ptr(), d_nfound.data_ptr())
        torch.cuda.synchronize()
        recs = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE).reshape(K, nb)
        count, corr = d_count.cpu().numpy(), d_corr.cpu().numpy()
        label, nfound = d_label.cpu().numpy(), d_nfound.cpu().numpy().astype(np.uint32)
        what = f"k={k} features form, layout {layout}"
        assert count.tolist() == [[len(s), 0] for s, _ in problems], what
        assert np.array_equal(corr[:, 0], ident) and np.array_equal(corr[:, 1], ident), what
        _assert_batch((recs, label, nfound, so), exp, what)
        assert recs.tobytes() == plain[0].tobytes() and np.array_equal(label, plain[1]) and np.array_equal(nfound, plain[2]), what
