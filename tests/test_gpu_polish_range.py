"""GPU: sc_polish at the ends of the fp32 range.

sc_polish.hip iterates inlier ballot, two-pass fp64 sums and solve inside one launch and stops on bitwise equality of consecutive
iterates; tests/test_gpu_polish.py runs it on the configs' own scenes, and tests/test_gpu_range.py::test_refine_and_peel covers ONE
refit at these magnitudes.  Here the iterated form, its candidate select and its stop rules run on test_range_oracle.scene_small
times 2^k, far from the origin, with rows at +-3e38 and with tau at the ends of its range, against tests/polish_ref.py through the
assertions of test_gpu_polish.py: every candidate's (R, t), rank, score0, score and iters, the winner, the mask, best_rank and
best_count, bit for bit.  tests/test_batch_range_ref.py owns the cases and asserts on the reference alone that they stop in every
way: at a fixed point, by a declined refit (before the first, and after several), at max_iter.
"""
import numpy as np
import pytest

import test_batch_range_ref as R
from conftest import nan_equal_bits
from test_gpu_polish import SC_ENOHYP, SC_OK, _assert_polish, _flat
from test_range_oracle import pow2

pytestmark = pytest.mark.gpu

_GPU = {}


def _polish(pkg, O, reg, name):
    """frame + polish of one case on the GPU, checked against the reference -> the polish result (None: the frame is SC_ENOHYP)"""
    src, tgt, kw, mode, frame, hyp, exp = R.polish_case_ref(pkg, O, name)
    k = R.polish_k(name)
    f = reg.register(src, tgt, params=pkg.make_params(**kw, score_mode=mode, flags=pkg.SC_FLAG_EXACT_TOTAL))
    st = f["stats"]
    print(name, "frame", f["status"], st["edges"], st["tri_total"], st["tri_kept"], st["best_rank"], st["best_count"], "| restatement", frame["rc"],
          frame["edges"], frame["tri_total"], frame["t_eff"], frame["best_rank"], frame["best_count"])
    assert f["status"] == frame["rc"], name
    assert (st["edges"], st["tri_total"], st["tri_kept"], st["best_rank"], st["best_count"]) == \
        (frame["edges"], frame["tri_total"], frame["t_eff"], frame["best_rank"], frame["best_count"]), name
    assert np.array_equal(f["mask"], frame["mask"]) and nan_equal_bits(f["R"], frame["R"]) and nan_equal_bits(f["t"], frame["t"]), name
    if f["status"] != SC_OK:                      # a frame call that returned SC_ENOHYP leaves no frame
        with pytest.raises(pkg.SacCotError) as e:
            reg.polish(candidates=k, max_iter=R.POLISH_ITERS)
        assert e.value.status == -1 and exp["status"] == SC_ENOHYP and not exp["cand"]
        return None
    got = reg.polish(candidates=k, max_iter=R.POLISH_ITERS)
    _assert_polish(got, exp, k, name)
    again = reg.polish(candidates=k, max_iter=R.POLISH_ITERS)
    assert again["cand"].tobytes() == got["cand"].tobytes() and _flat(again).tobytes() == _flat(got).tobytes(), name
    return got


@pytest.mark.parametrize("name", R.POLISH_CASES)
def test_polish_equals_the_reference_at_the_ends_of_the_range(pkg, O, reg, name):
    _GPU[name] = _polish(pkg, O, reg, name)
    if name == "f:tau-30":
        assert _GPU[name] is None
    if name == "c:20:22":                         # a limit that bites, on iterates that wander (quantised coordinates)
        src, tgt, kw, mode, frame, hyp, exp = R.polish_case_ref(pkg, O, name)
        assert max(int(c["iters"]) for c in _GPU[name]["cand"]) == R.POLISH_ITERS


def test_inside_the_window_the_gpu_equals_itself_at_unit_scale(pkg, O, reg):
    """Without the oracle: every candidate at k is the candidate at k = 0 with t times 2^k (tests/test_batch_range_ref.py: the
    reference is covariant at these k)."""
    def gpu(k):
        name = f"a:{k}"
        if name not in _GPU:
            _GPU[name] = _polish(pkg, O, reg, name)
        return _GPU[name]
    g0 = gpu(0)
    ks = R.polish_metamorphic_ks()
    assert len(ks) >= 3 and g0["n_cand"] == R.POLISH_K
    for k in ks:
        g = gpu(k)
        assert g["status"] == g0["status"] and g["n_cand"] == g0["n_cand"], k
        for f in ("rank", "score0", "score", "iters"):
            assert np.array_equal(g["cand"][f], g0["cand"][f]), (k, f)
        assert g["cand"]["Rt"][:, :9].tobytes() == g0["cand"]["Rt"][:, :9].tobytes(), k
        assert g["cand"]["Rt"][:, 9:].tobytes() == (g0["cand"]["Rt"][:, 9:] * pow2(k)).tobytes(), k
        assert g["R"].tobytes() == g0["R"].tobytes() and g["t"].tobytes() == (g0["t"] * pow2(k)).tobytes(), k
        assert np.array_equal(g["mask"], g0["mask"]), k
        assert (g["stats"]["best_rank"], g["stats"]["best_count"]) == (g0["stats"]["best_rank"], g0["stats"]["best_count"]), k
