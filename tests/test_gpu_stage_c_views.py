"""GPU: the views of the context's stage-C arrays (sc_kernels.hpp: Hyps, FilterBufs, Partial) across a frame that grows them.

A view holds plain pointers; a buffer that grows is freed and allocated again.  The host driver takes every view behind the last
ENSURE of what it names — a view kept across one would hand a launch the freed address.  This test makes every buffer of stage C
grow between two frames of ONE context and compares what follows with a context that has seen the second frame only.

Per forced C2 kernel (sc_debug.score_filter = 3 Gram filter, 2 linear filter, 1 plain fp32 kernel), on the same context:
  a small frame   n = 200,  max_triangles = 300  (ld_local 512);
  a larger frame  n = 1100, max_triangles = 1500 (ld_local 1536; n crosses one 1024-correspondence window of the filters),
  then sc_peel twice, sc_polish, and sc_score_host on the frame's hypotheses.
The Gram filter goes first because it is the one that uses all six arrays: with a buffer's smallest allocation at 64 KiB, the second
frame then grows rt and rt_aos (24 -> 72 KiB asked), fx_tile (80 -> 144 KiB), fx_coef (45 -> 129 KiB), fx_state (the small frame runs
with filter_queue_cap = 256: 35 -> 545 KiB) under the frame's launches and partial (the filters ask 12 KiB, the plain kernel of the
first sc_peel round 90 KiB) under the round's; the linear filter's own tile and the plain kernel then meet arrays of another
mode's sizes.  Every R, t, mask, count and key must equal, bit for bit, what the fresh context gives for the same call.
"""
import numpy as np
import pytest

from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SMALL = dict(n=200, T=300, seed=4101)
LARGE = dict(n=1100, T=1500, seed=4102)
L, TAU = 1.0, 0.05


def _frame(pkg, n, T, seed):
    sc = pkg.synth.make_scene_motions(n, [0.18, 0.12], L, TAU, seed)
    return sc.src, sc.tgt, pkg.make_params(sigma=TAU, t_cmp=0.90, tau=TAU, min_len=TAU, max_triangles=T, rank_mode=0)


_HYPS = {}


def _hypotheses(pkg):
    """The larger frame's hypotheses (ranked list -> Kabsch through the stage hooks of a context of their own), once per session."""
    if "Rt" not in _HYPS:
        src, tgt, p = _frame(pkg, **LARGE)
        helper = pkg.Registrar(0)
        tri = helper.triangles(src, tgt, p)[0]
        _HYPS["Rt"] = helper.kabsch(src, tgt, p, tri)
        helper.close()
    return _HYPS["Rt"]


def _after_large_frame(pkg, reg):
    """The larger frame and everything the test runs behind it, as (name, result) pairs."""
    src, tgt, p = _frame(pkg, **LARGE)
    out = [("register", reg.register(src, tgt, params=p)), ("peel 1", reg.peel()), ("peel 2", reg.peel()),
           ("polish", reg.polish(candidates=8, max_iter=16))]
    cnt, key = reg.score(src, tgt, p, _hypotheses(pkg))
    return out, cnt, key


def _assert_same(name, got, exp):
    print(name, "status", got["status"], exp["status"], "rank", got["stats"]["best_rank"], exp["stats"]["best_rank"],
          "count", got["stats"]["best_count"], exp["stats"]["best_count"], "inliers", int(got["mask"].sum()), int(exp["mask"].sum()))
    assert got["status"] == exp["status"], name
    assert nan_equal_bits(got["R"], exp["R"]) and nan_equal_bits(got["t"], exp["t"]), name
    assert np.array_equal(got["mask"], exp["mask"]), name
    for k in ("best_rank", "best_count", "tri_kept"):
        assert got["stats"][k] == exp["stats"][k], (name, k)
    if "cand" in exp:
        assert got["n_cand"] == exp["n_cand"], name
        assert got["cand"].tobytes() == exp["cand"].tobytes(), name


def test_views_follow_the_arrays_when_a_frame_grows_them(pkg):
    reg = pkg.Registrar(0)
    for mode in (3, 2, 1):
        reg.set_debug(score_filter=mode, filter_queue_cap=256)
        src, tgt, p = _frame(pkg, **SMALL)
        small = reg.register(src, tgt, params=p)
        assert small["status"] == 0 and small["stats"]["tri_kept"] == SMALL["T"], "the small frame must fill its 300 hypotheses"
        assert reg.debug_last()["c2_kernel"] == mode - 1, "the forced C2 kernel must be the one that ran"
        reg.set_debug(score_filter=mode)
        got, cnt, key = _after_large_frame(pkg, reg)
        assert got[0][1]["stats"]["tri_kept"] == LARGE["T"], "the larger frame must fill its 1500 hypotheses (ld_local 1536)"

        fresh = pkg.Registrar(0)
        fresh.set_debug(score_filter=mode)
        exp, cnt_exp, key_exp = _after_large_frame(pkg, fresh)
        fresh.close()
        for (name, g), (_, e) in zip(got, exp):
            _assert_same(f"score_filter={mode} {name}", g, e)
        print(f"score_filter={mode} score hook: key {key:#x} {key_exp:#x}, counts differing {int((cnt != cnt_exp).sum())}")
        assert key == key_exp and np.array_equal(cnt, cnt_exp), f"score_filter={mode} sc_score_host"
        assert got[0][1]["status"] == 0 and key != 0, "the comparison must be of real results"
    reg.close()
