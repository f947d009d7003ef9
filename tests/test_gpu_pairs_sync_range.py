"""GPU: sc_pairs_sync at the ends of the fp32 range, on its rotation cut and to its round limit (include/saccot.h).

tests/test_gpu_pairs_sync.py hands the entry rotations with translations of order 1 .. 10 and weights in [1e-3, 4], sits on the
translation cut only, and never runs max_rounds 1 or 256.  These families do the rest (tests/sync_ref.py; tests/test_sync_abi.py
checks on the CPU that they are what they are used for, and holds what the reference measures on them as literals):

  rcut           set 1 turns by exactly dR2 = 8.0 = r2_max at rot_tol 2.0; sets 2 and 3, known, meet a sum of rank one.
  exact24, ring  cube rotations and integer translations: the expected poses are np.int64 products that share no code with the
                 reference, every residual is exactly 0.0.
  scaled         the translations and trans_tol times 2^k, the weights times 2^k: what must not move, and what moves by 2^k or 4^k
                 exactly, is asserted on the device's own two outputs.
  weights_range  weights from 1e-45 to FLT_MAX.
  hostile        finite records that are no rotations, over the whole exponent range: |X.t| up to 4e76, Rt infinite in 69 components.
  ring40         256 rounds run to the limit, a stop on the device with 136 launches behind it, and one round.
  sparse         8200 sets of which 42 have a list.
  self_star      the set records of one call as the pose records of the next, in place — hostile's, with their infinities, too.

As there, every comparison is bit for bit against sync_ref.sync fed the thresholds the library derives.  No tolerances.
"""
import numpy as np
import pytest

import sync_ref as SR
import test_sync_abi as ABI  # the literals
from test_gpu_pairs_sync import PAIR, SET, SUM, _assert_same, _device, _expected, _fetch, _host, _params, _records

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5


def _both_forms(pkg, reg, f, sp, exp, what, stride=48, statuses=None):
    """the device and the host form on family f -> the device form's result"""
    raw = _records(f.rt, stride, statuses)
    got = _device(pkg, reg, f.n_sets, f.pairs, sp, raw, use=f.use, weight=f.weight)
    _assert_same(got, exp, what + ", device form")
    _assert_same(_host(pkg, reg, f.n_sets, f.pairs, sp, raw, use=f.use, weight=f.weight), exp, what + ", host form")
    return got


def _exp(pkg, f, sp):
    return _expected(pkg, f, sp, use=f.use, weight=f.weight, statuses=f.statuses if sp.flags else None)


# ---- the rotation cut, and a known set that meets a degenerate sum ---------------------------------------------------------------------
@pytest.mark.parametrize("tol", list(ABI.RCUT_ROUNDS))
def test_a_set_on_the_rotation_cut_is_quiet(pkg, reg, tol):
    f = SR.rcut()
    sp = _params(pkg, f, rot_tol=tol)
    assert pkg.sync_thresholds(sp) == SR.thresholds(tol, 0.0) and (pkg.sync_thresholds(sp)[0] == 8.0) == (tol == SR.RCUT_TOL)
    got = _both_forms(pkg, reg, f, sp, _exp(pkg, f, sp), f"rcut, rot_tol {tol!r}")
    assert (int(got[2]["rounds"]), int(got[2]["converged"])) == ABI.RCUT_ROUNDS[tol]  # (test_sync_abi.py: dR2 == r2_max == 8.0 in round 2)
    assert got[0]["degenerate"].tolist() == ABI.RCUT_DEGENERATE and got[0]["used"].tolist() == ABI.RCUT_USED
    assert got[0]["X"][1][:9].tolist() == ABI.RCUT_R1 and (got[0]["status"] == SC_OK).all()  # sets 2 and 3 keep their pose and stay known
    assert got[0]["X"][2].tolist() == got[0]["X"][3].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


# ---- exact in integers: an expectation that shares no code with the reference --------------------------------------------------------------
@pytest.mark.parametrize("name,anchor", [("exact24", 0), ("exact24", 13), ("exact_ring", 0)])
def test_exact_worlds_equal_the_integers(pkg, reg, name, anchor):
    f = SR.exact24(anchor) if name == "exact24" else SR.exact_ring()
    sp = _params(pkg, f)
    assert sp.anchor == anchor and pkg.sync_thresholds(sp) == (0.0, 0.0)
    got = _both_forms(pkg, reg, f, sp, _exp(pkg, f, sp), f"{name}, anchor {anchor}")
    want = SR.integers(f, anchor)
    assert want.dtype == np.int64 and (got[0]["X"] == want).all() and (got[0]["Rt"] == want).all()
    assert got[1]["r2"].tobytes() == got[1]["e2"].tobytes() == bytes(8 * len(f.pairs)) and (got[1]["used"] == 1).all()  # +0.0 each
    summary = tuple(int(got[2][n]) for n in ("rounds", "converged", "known", "used"))
    assert summary == (ABI.EXACT24_SUMMARY if name == "exact24" else ABI.EXACT_RING_SUMMARY)
    if name == "exact_ring":
        assert got[0]["known_round"].tolist() == ABI.EXACT_RING_HOPS


# ---- scaled: the exponent range of the translations and of the weights -------------------------------------------------------------------
_GPU0 = {}  # the GPU's own results at scale 0, fetched once and never written


def _gpu0(pkg, reg, name, f):
    if name not in _GPU0:
        _GPU0[name] = _device(pkg, reg, f.n_sets, f.pairs, _params(pkg, f), _records(f.rt, 48), weight=f.weight)
    return _GPU0[name]


@pytest.mark.parametrize("k", SR.SCALES_EXACT + (SR.SCALE_UNDER,))
def test_scaled_translations(pkg, reg, k):
    g = SR.scaled(k)
    sp = _params(pkg, g)
    exp = _exp(pkg, g, sp)
    got = _both_forms(pkg, reg, g, sp, exp, f"k24 x 2^{k}")
    if k == SR.SCALE_UNDER:  # the floats are subnormal and rounded: only the reference applies
        assert tuple(int(got[2][n]) for n in ("rounds", "converged", "known", "used", "changed_last")) == ABI.SCALE_UNDER_SUMMARY
        return
    sets0, pairs0, s0 = _gpu0(pkg, reg, "k24", SR.k24())
    sets, pairs, s = got
    assert s.tobytes() == s0.tobytes() and tuple(int(s[n]) for n in ("rounds", "converged", "known", "used")) == ABI.K24_SUMMARY
    assert sets["X"][:, :9].tobytes() == sets0["X"][:, :9].tobytes() and sets["Rt"][:, :9].tobytes() == sets0["Rt"][:, :9].tobytes()
    assert sets["X"][:, 9:].tobytes() == np.ldexp(sets0["X"][:, 9:], k).tobytes()
    assert pairs["r2"].tobytes() == pairs0["r2"].tobytes() and pairs["e2"].tobytes() == np.ldexp(pairs0["e2"], 2 * k).tobytes() and (pairs["e2"] > 0).all()
    for name in ("status", "known_round", "used", "degenerate"):
        assert sets[name].tobytes() == sets0[name].tobytes(), name
    assert pairs["status"].tobytes() == pairs0["status"].tobytes() and pairs["used"].tobytes() == pairs0["used"].tobytes()


@pytest.mark.parametrize("k", [-100, 100, SR.SCALE_UNDER])
def test_scaled_weights(pkg, reg, k):
    g = SR.weight_scaled(k)
    sp = _params(pkg, g)
    got = _both_forms(pkg, reg, g, sp, _exp(pkg, g, sp), f"weights x 2^{k}")
    summary = tuple(int(got[2][n]) for n in ("rounds", "converged", "known", "used"))
    if k == SR.SCALE_UNDER:  # weights go subnormal or to zero: only the reference applies
        assert summary == ABI.WEIGHT_UNDER[0]
        return
    base = _gpu0(pkg, reg, "weights", SR.weight_scaled(0))
    assert summary == ABI.WEIGHT_SCALED_SUMMARY and all(a.tobytes() == b.tobytes() for a, b in zip(got, base))  # every output byte


# ---- weights and records over the whole fp32 range -----------------------------------------------------------------------------------------
def test_weights_over_the_whole_range(pkg, reg):
    g = SR.weights_range()
    sp = _params(pkg, g)
    got = _both_forms(pkg, reg, g, sp, _exp(pkg, g, sp), "weights_range")
    assert tuple(int(got[2][n]) for n in ("rounds", "converged", "known", "used", "changed_last")) == ABI.WEIGHTS_RANGE_SUMMARY
    assert not got[0]["degenerate"].any() and np.isfinite(got[0]["X"]).all() and np.flatnonzero(got[1]["used"] == 0).tolist() == [101, 202]


@pytest.mark.parametrize("anchor,max_rounds", list(ABI.HOSTILE))
def test_hostile_records(pkg, reg, anchor, max_rounds):
    f = SR.hostile()
    summary, degenerate, not_finite = ABI.HOSTILE[(anchor, max_rounds)]
    st = np.zeros(len(f.pairs), np.int32)
    exp = _expected(pkg, f, _params(pkg, f, anchor=anchor, max_rounds=max_rounds))  # (status words that are all SC_OK change nothing)
    for stride, flags in ((48, 0), (64, pkg.SC_SYNC_STATUS)):
        sp = _params(pkg, f, anchor=anchor, max_rounds=max_rounds, flags=flags)
        got = _both_forms(pkg, reg, f, sp, exp, f"hostile, anchor {anchor}, max_rounds {max_rounds}, stride {stride}", stride, st if flags else None)
        assert tuple(int(got[2][n]) for n in ("rounds", "converged", "known", "used", "changed_last")) == summary
        assert np.flatnonzero(got[0]["degenerate"]).tolist() == degenerate and (got[0]["degenerate"] <= 1).all()
        # every X is finite and Rt, X rounded once to fp32, is not: under SC_OK (the header says so)
        assert np.isfinite(got[0]["X"]).all() and int((~np.isfinite(got[0]["Rt"])).sum()) == not_finite and not np.isnan(got[0]["Rt"]).any()
        assert (got[0]["status"] == SC_OK).all() and (got[1]["status"] == SC_OK).all()
        assert np.isfinite(got[1]["r2"]).all() and np.isfinite(got[1]["e2"]).all()


# ---- to the round limit, and a stop on the device far ahead of it -----------------------------------------------------------------------------
@pytest.mark.parametrize("tol,max_rounds", list(ABI.RING40))
def test_the_ring_of_40(pkg, reg, tol, max_rounds):
    f = SR.ring40()
    sp = _params(pkg, f, rot_tol=tol, trans_tol=tol, max_rounds=max_rounds)
    got = _both_forms(pkg, reg, f, sp, _exp(pkg, f, sp), f"ring40, tolerances {tol}, max_rounds {max_rounds}")
    assert tuple(int(got[2][n]) for n in ("rounds", "converged", "known", "used", "changed_last")) == ABI.RING40[(tol, max_rounds)]
    if max_rounds == 1:
        assert np.flatnonzero(got[0]["status"] == SC_OK).tolist() == [0, 1, 39]


def test_sets_with_empty_lists_past_the_grid(pkg, reg):
    f = SR.sparse()
    sp = _params(pkg, f)
    got = _both_forms(pkg, reg, f, sp, _exp(pkg, f, sp), "sparse")
    assert tuple(int(got[2][n]) for n in ("rounds", "converged", "known", "used", "changed_last")) == ABI.SPARSE_SUMMARY
    assert (got[0]["status"] == SC_ENOHYP).sum() == f.n_sets - 42 and not got[0]["X"][42:].any()


# ---- a result as the next call's pose records ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ABI.SELF_STAR))
def test_a_result_is_an_array_of_pose_records(pkg, reg, name):
    import torch
    f = getattr(SR, name)()
    anchor, summary = ABI.SELF_STAR[name]
    sp1 = _params(pkg, f, anchor=anchor)
    exp1 = _exp(pkg, f, sp1)
    g = SR.self_star(exp1[0], anchor)  # the list and the parameters; the second call's records are the device's own
    sp2 = _params(pkg, g)
    assert sp2.flags == pkg.SC_SYNC_STATUS and sp2.anchor == anchor
    exp2 = _exp(pkg, g, sp2)
    d_pose = torch.from_numpy(_records(f.rt, 48).reshape(-1).copy()).cuda()
    out = [[torch.full((n * size,), fill, dtype=torch.uint8, device="cuda") for n, size, fill in ((f.n_sets, SET, 0xAB), (len(pairs), PAIR, 0xAC), (1, SUM, 0xCD))]
           for pairs in (f.pairs, g.pairs)]
    torch.cuda.synchronize()
    reg.pairs_sync_device(f.n_sets, f.pairs, sp1, d_pose.data_ptr(), 48, 0, 4, 0, *(t.data_ptr() for t in out[0]))
    reg.pairs_sync_device(g.n_sets, g.pairs, sp2, out[0][0].data_ptr(), SET, 0, 4, 0, *(t.data_ptr() for t in out[1]))  # no wait, no host copy
    torch.cuda.synchronize()
    first, second = _fetch(pkg, *out[0]), _fetch(pkg, *out[1])
    _assert_same(first, exp1, f"{name}, the first call")
    _assert_same(second, exp2, f"{name}, the second call over the first one's records")
    assert tuple(int(second[2][n]) for n in ("rounds", "converged", "known", "used")) == summary
    # SC_ENOHYP passes through, and a record with an infinite Rt is SC_EINVAL under its SC_OK: a pose entry — this one — rules so
    finite = np.isfinite(first[0]["Rt"]).all(axis=1)
    assert (second[1]["status"] == np.where((first[0]["status"] == SC_OK) & ~finite, SC_EINVAL, first[0]["status"])).all()
    assert (second[0]["status"] == np.where((first[0]["status"] == SC_OK) & finite, SC_OK, SC_ENOHYP)).all()
    assert ((first[0]["status"] == SC_ENOHYP).sum(), (~finite).sum()) == {"k24": (0, 0), "two_components": (6, 0), "hostile": (0, 23)}[name]


# ---- two device-form calls on one context, nothing waited for in between ----------------------------------------------------------------------
@pytest.mark.parametrize("order", ["the second grows the workspace", "the second reuses it", "other round limits"])
def test_two_calls_back_to_back(pkg, order):
    import torch
    small, big = SR.chain(), SR.g512()
    calls = {"the second grows the workspace": ((small, 64), (big, 32)), "the second reuses it": ((big, 32), (small, 64)),
             "other round limits": ((small, 42), (small, 3))}[order]
    sps = [_params(pkg, f, max_rounds=m) for f, m in calls]
    exps = [_exp(pkg, f, sp) for (f, _m), sp in zip(calls, sps)]
    poses = [torch.from_numpy(_records(f.rt, 48).reshape(-1).copy()).cuda() for f, _m in calls]
    outs = [[torch.full((n * size,), fill, dtype=torch.uint8, device="cuda") for n, size, fill in ((f.n_sets, SET, 0xAB), (len(f.pairs), PAIR, 0xAC), (1, SUM, 0xCD))]
            for f, _m in calls]
    torch.cuda.synchronize()
    fresh = pkg.Registrar(0)
    try:
        for (f, _m), sp, d_pose, out in zip(calls, sps, poses, outs):
            fresh.pairs_sync_device(f.n_sets, f.pairs, sp, d_pose.data_ptr(), 48, 0, 4, 0, *(t.data_ptr() for t in out))
        torch.cuda.synchronize()
        for i, (exp, out) in enumerate(zip(exps, outs)):
            _assert_same(_fetch(pkg, *out), exp, f"{order}: call {i + 1}")
    finally:
        torch.cuda.synchronize()
        fresh.close()
    if order == "other round limits":  # the first call's round words say "stopped at 42"; the second must end at its own limit
        assert [(int(e[2]["rounds"]), int(e[2]["converged"]), int(e[2]["known"])) for e in exps] == [(42, 1, 42), (3, 0, 4)]
