"""GPU: pose-gated matching for listed pairs of shared keypoint sets (include/saccot.h, sc_match_guided_pairs /
sc_match_guided_pairs_device / sc_register_guided_pairs_features_device).

Pair p's outputs are the packed guided entries' for problem p of the list EXPANDED into packed problems in list order, under pose
record p: every comparison is bit for bit against that expansion through sc_match_guided_batch_device and against the numpy
restatement (tests/match_guided_batch_ref.py).  tests/test_match_guided_batch_abi.py checks the table and the list on the CPU.
"""
import numpy as np
import pytest

import match_batch_ref as M
import match_guided_batch_ref as GB
import match_guided_ref as MG

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5


@pytest.fixture(scope="module")
def greg(pkg):
    r = pkg.Registrar(0)
    yield r
    r.close()


def _run_pairs(pkg, r, tab, pairs, poses, gate, flags=0, layout=0, want_g2=True, **mkw):
    """sc_match_guided_pairs_device on the current torch stream -> (corr, d2, g2 or None, count)"""
    import torch
    m = pkg.api.make_match_params(tab["feat"].shape[1], **mkw)
    g = pkg.make_guide_params(gate, layout, flags)
    pose, stride = r._pose_records(poses, len(pairs))
    pts = tab["pts"] if layout == 0 else np.ascontiguousarray(tab["pts"].T)
    d = GB.to_device((pts, tab["feat"], pose.view(np.uint8).reshape(-1)))
    slots = int(r.pairs_layout(tab["set_off"], pairs, m.knn)[-1])
    out = GB.outputs(slots, len(pairs))
    torch.cuda.synchronize()
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        r.match_guided_pairs_device(d[0].data_ptr(), d[1].data_ptr(), tab["set_off"], pairs, m, g, d[2].data_ptr(), stride, out[0].data_ptr(),
                                    out[1].data_ptr(), out[2].data_ptr() if want_g2 else None, out[3].data_ptr())
        torch.cuda.synchronize()
    finally:
        r.set_stream(None)
    return GB.fetch(out, slots, len(pairs), want_g2)


def test_every_pair_equals_the_packed_entry_and_the_restatement(pkg, greg):
    tab = GB.table()
    eb = GB.expand(tab, GB.PAIRS, tab["poses"])
    for kw in MG.MODES:
        for layout in (0, pkg.SC_SOA):
            exp = GB.match_batch(eb, MG.GATE, **kw)
            got = _run_pairs(pkg, greg, tab, GB.PAIRS, tab["poses"], MG.GATE, layout=layout, **kw)
            GB.same(got, exp, ("pairs", kw, layout))
            packed = GB.run_device(pkg, greg, eb, MG.GATE, layout=layout, **kw)
            for k in range(4):
                assert got[k].tobytes() == packed[k].tobytes(), (kw, layout, k)
        assert (got[3][:, 0] > 0).all() and got[3][0].tolist() != got[3][2].tolist()  # the pair listed twice: two poses, two answers
    # the host form, with and without g2, and the records with a status: a skipped pair between its neighbours
    statuses = np.zeros(len(GB.PAIRS), np.int32); statuses[2] = SC_ENOHYP
    rec = eb.poses(GB.POSE80, statuses=statuses)
    exp = GB.match_batch(eb, MG.GATE, statuses=statuses, knn=2)
    GB.same(_run_pairs(pkg, greg, tab, GB.PAIRS, rec, MG.GATE, flags=GB.STATUS, knn=2), exp, "pairs, a skipped pair")
    for want_g2 in (True, False):
        corr, d2, g2, count, slot = greg.match_guided_pairs(tab["pts"], tab["feat"], tab["set_off"], GB.PAIRS, rec, gate=MG.GATE, flags=GB.STATUS,
                                                            want_g2=want_g2, knn=2)
        assert np.array_equal(count, exp[3]) and (g2 is None) == (not want_g2)
        for p in range(len(GB.PAIRS)):
            lo, n = int(slot[p]), int(count[p, 0])
            assert corr[lo: lo + n].tobytes() == exp[0][lo: lo + n].tobytes() and d2[lo: lo + n].tobytes() == exp[1][lo: lo + n].tobytes(), p
            assert g2 is None or g2[lo: lo + n].tobytes() == exp[2][lo: lo + n].tobytes(), p


def test_a_non_finite_value_flags_the_pairs_that_use_its_set(pkg, greg):
    import pairs_ref
    tab = GB.table()
    clean = _run_pairs(pkg, greg, tab, GB.PAIRS, tab["poses"], MG.GATE, knn=1, mutual=True)
    slot = greg.pairs_layout(tab["set_off"], GB.PAIRS, 1)
    for s, which, pos, val in ((3, 1, (100, 32), np.nan), (0, 0, (64, 2), np.inf), (4, 1, (0, 0), -np.inf)):
        arrs = [tab["sets"][s][0].copy(), tab["sets"][s][1].copy()]
        arrs[which][pos] = val
        bad = dict(pairs_ref.with_sets(tab, {s: tuple(arrs)}), poses=tab["poses"])
        got = _run_pairs(pkg, greg, bad, GB.PAIRS, tab["poses"], MG.GATE, knn=1, mutual=True)
        uses = np.array([s in pr for pr in GB.PAIRS.tolist()])
        print("set", s, "pairs flagged", got[3][:, 1].tolist())
        assert uses.any() and not uses.all() and got[3][:, 1].tolist() == uses.astype(int).tolist() and not got[3][uses, 0].any()
        GB.same(got, GB.match_batch(GB.expand(bad, GB.PAIRS, tab["poses"]), MG.GATE, knn=1, mutual=True), ("a bad set", s))
        for p in np.flatnonzero(~uses):  # the others: bit for bit what they were
            lo, hi = int(slot[p]), int(slot[p + 1])
            for k in range(3):
                assert got[k][lo:hi].tobytes() == clean[k][lo:hi].tobytes(), (s, p, k)


def test_register_guided_pairs_features_equals_the_packed_entry(pkg, greg):
    import torch
    tab = GB.table()
    eb = GB.expand(tab, GB.PAIRS, tab["poses"])
    npairs = len(GB.PAIRS)
    mp, p = pkg.api.make_match_params(tab["feat"].shape[1]), pkg.make_params(**M.KW)
    g = pkg.make_guide_params(MG.GATE)
    so, to = eb.offsets()
    slots = int(so[-1])

    def outs():
        return GB.outputs(slots, npairs), torch.zeros(npairs * 80, dtype=torch.uint8, device="cuda"), torch.full((slots,), 7, dtype=torch.uint8, device="cuda")

    d_pose = GB.to_device((tab["poses"],))[0]
    dt = GB.to_device((tab["pts"], tab["feat"]))
    de = GB.to_device(eb.packed())
    (a_out, a_res, a_mask), (b_out, b_res, b_mask) = outs(), outs()
    torch.cuda.synchronize()
    greg.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        greg.register_guided_pairs_features_device(dt[0].data_ptr(), dt[1].data_ptr(), tab["set_off"], GB.PAIRS, mp, g, d_pose.data_ptr(), 48, p,
                                                   a_res.data_ptr(), a_out[0].data_ptr(), a_out[1].data_ptr(), a_out[2].data_ptr(),
                                                   a_out[3].data_ptr(), a_mask.data_ptr())
        greg.register_guided_batch_features_device(de[0].data_ptr(), de[1].data_ptr(), so, de[2].data_ptr(), de[3].data_ptr(), to, mp, g,
                                                   d_pose.data_ptr(), 48, p, b_res.data_ptr(), b_out[0].data_ptr(), b_out[1].data_ptr(),
                                                   b_out[2].data_ptr(), b_out[3].data_ptr(), b_mask.data_ptr())
        torch.cuda.synchronize()
    finally:
        greg.set_stream(None)
    a, b = GB.fetch(a_out, slots, npairs), GB.fetch(b_out, slots, npairs)
    GB.same(a, GB.match_batch(eb, MG.GATE), "the pairs features entry's match")
    for k in range(4):
        assert a[k].tobytes() == b[k].tobytes(), k
    ra, rb = a_res.cpu().numpy().view(GB.POSE80), b_res.cpu().numpy().view(GB.POSE80)
    print("statuses", ra["status"].tolist(), "n", ra["n"].tolist())
    assert ra.tobytes() == rb.tobytes() and (ra["n"] == a[3][:, 0]).all()
    ma, mb = a_mask.cpu().numpy(), b_mask.cpu().numpy()
    for q in range(npairs):
        lo, n = int(so[q]), int(a[3][q, 0])
        assert ma[lo: lo + n].tobytes() == mb[lo: lo + n].tobytes(), q
