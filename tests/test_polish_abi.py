"""CPU suite: the surface of sc_polish (include/saccot.h) — the three exports, the Python mirror, the struct layout, the argument
checks that need no GPU — and the numpy restatement of its semantics (tests/polish_ref.py) that the GPU tests compare against,
checked here for what it promises on the C1 scene.  No compute call reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polish_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_polish_default_params", "sc_polish_device", "sc_polish")
SC_EINVAL = -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_polish_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("polish", "polish_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.ScPolishParams is pkg.api.ScPolishParams and pkg.ScPolishCand is pkg.api.ScPolishCand
    assert callable(pkg.make_polish_params)


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_POLISH 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_polish_struct_layouts_and_defaults(pkg):
    exe = os.path.join(ROOT, "tests", ".abi_probe_polish")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", '
           'sizeof(sc_polish_params), offsetof(sc_polish_params, candidates), offsetof(sc_polish_params, max_iter), '
           'offsetof(sc_polish_params, reserved), sizeof(sc_polish_cand), offsetof(sc_polish_cand, rank), offsetof(sc_polish_cand, score0), '
           'offsetof(sc_polish_cand, score), offsetof(sc_polish_cand, iters), sizeof(sc_stats));return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    finally:
        os.remove(exe)
    P, K = pkg.api.ScPolishParams, pkg.api.ScPolishCand
    assert got[:4] == [32, P.candidates.offset, P.max_iter.offset, P.reserved.offset] and C.sizeof(P) == 32
    assert got[4:9] == [64, K.rank.offset, K.score0.offset, K.score.offset, K.iters.offset] and C.sizeof(K) == 64
    assert got[9] == C.sizeof(pkg.ScStats)  # sc_stats did not move
    dt = pkg.api.POLISH_CAND_DTYPE
    assert dt.itemsize == 64 and [dt.fields[k][1] for k in ("Rt", "rank", "score0", "score", "iters")] == [0, 48, 52, 56, 60]
    L = pkg.load_library()
    p = P()
    assert L.sc_polish_default_params(C.byref(p)) == 0  # (host only: no GPU needed)
    assert (p.size, p.candidates, p.max_iter, p.flags, list(p.reserved)) == (32, 8, 16, 0, [0, 0, 0, 0])
    assert L.sc_polish_default_params(None) == SC_EINVAL
    q = pkg.make_polish_params()
    assert bytes(q) == bytes(p)
    q = pkg.make_polish_params(candidates=3, max_iter=5)
    assert (q.size, q.candidates, q.max_iter, q.flags) == (32, 3, 5, 0)


def test_null_arguments_are_refused_without_a_gpu(pkg):
    L = pkg.load_library()
    p = pkg.make_polish_params()
    R = (C.c_float * 9)(); t = (C.c_float * 3)(); mask = (C.c_uint8 * 8)(); st = pkg.ScStats(C.sizeof(pkg.ScStats))
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on a NULL before it looks at anything else
    assert L.sc_polish(None, C.byref(p), R, t, mask, None, None, C.byref(st)) == SC_EINVAL
    assert L.sc_polish_device(None, C.byref(p), fake, fake, None, None, C.byref(st)) == SC_EINVAL
    # (a context cannot exist here — sc_create fails without a GPU — so the NULL outputs are tried with a NULL context too; the
    # GPU suite repeats them on a real one)
    assert L.sc_polish(None, C.byref(p), None, t, mask, None, None, None) == SC_EINVAL
    assert L.sc_polish(None, None, R, t, mask, None, None, None) == SC_EINVAL
    assert L.sc_polish_device(None, C.byref(p), None, None, None, None, None) == SC_EINVAL


# ---- what the restatement promises on C1 with the config's own parameters -------------------------------------------------
_C1 = {}


def _c1(pkg, O):
    if not _C1:
        cfg, sc = pkg.synth.make_config_scene("C1")
        kw = cfg.params()
        th = min(O.max_threads(), 16)
        _C1.update(cfg=cfg, sc=sc, kw=kw, th=th, hyp=polish_ref.hypotheses(O, sc.src, sc.tgt, kw, th))
    return _C1


def _errors(pkg, sc, rt):
    R, t = rt[:9].reshape(3, 3).astype(np.float64), rt[9:].astype(np.float64)
    return pkg.synth.rotation_error_deg(R, sc.R_gt), float(np.linalg.norm(t - sc.t_gt))


def _run(pkg, O, tau, mode, k=4, iters=16):
    c = _c1(pkg, O)
    Rt = c["hyp"]["Rt"]
    cnt = O.score(c["sc"].src, c["sc"].tgt, Rt, tau, threads=c["th"], score_mode=mode)
    res = polish_ref.polish(O, c["sc"].src, c["sc"].tgt, Rt, tau, mode, k, iters, cnt=cnt)
    g0 = polish_ref.candidates(cnt, 1)[0]
    return res, int(cnt[g0]), Rt[g0]


def test_reference_reaches_a_fixed_point_and_a_better_pose_on_c1(pkg, O):
    c = _c1(pkg, O)
    res, raw_count, raw_rt = _run(pkg, O, c["kw"]["tau"], 0)
    print("count mode:", raw_count, _errors(pkg, c["sc"], raw_rt), "->", res["best_count"], _errors(pkg, c["sc"], res["Rt"]),
          [(k["rank"], k["score0"], k["score"], k["iters"], k["stop"]) for k in res["cand"]])
    assert res["status"] == 0 and len(res["cand"]) == 4
    assert all(k["stop"] == "fixed" and k["iters"] < 16 for k in res["cand"])
    assert res["cand"][0]["score0"] == raw_count and [k["score0"] for k in res["cand"]] == sorted((k["score0"] for k in res["cand"]), reverse=True)
    (rot1, tr1), (rot0, tr0) = _errors(pkg, c["sc"], res["Rt"]), _errors(pkg, c["sc"], raw_rt)
    assert rot1 < rot0 and tr1 < tr0
    assert res["mask"].sum() == res["best_count"]  # inlier-count mode


def test_reference_raises_the_truncated_score_on_c1(pkg, O):
    c = _c1(pkg, O)
    res, raw, _ = _run(pkg, O, c["kw"]["tau"], 1)
    print("MSE mode:", raw, "->", res["best_count"])
    assert res["best_count"] > raw


def test_reference_raises_the_count_at_half_tau_on_c1(pkg, O):
    c = _c1(pkg, O)
    res, raw, _ = _run(pkg, O, c["kw"]["tau"] / 2, 0, k=8)
    print("count mode, tau / 2:", raw, "->", res["best_count"], "winner", res["winner"], [(k["score0"], k["score"], k["iters"]) for k in res["cand"]])
    assert res["best_count"] > raw and res["best_count"] >= 201
    assert max(k["iters"] for k in res["cand"]) >= 9  # what the GPU test of this case relies on: many refits in one launch


def test_the_scenes_of_the_gpu_tests_are_what_they_are_used_for(pkg, O):
    for n in (64, 65, 129):  # the chunk edges: a frame and a polish exist for each
        kw, src, tgt = polish_ref.edge_scene(pkg, n)
        hyp = polish_ref.hypotheses(O, src, tgt, kw)
        res = polish_ref.polish(O, src, tgt, hyp["Rt"], kw["tau"], 0, 8, 16)
        assert src.shape == (n, 3) and res["status"] == 0 and len(res["cand"]) == 8 and max(k["iters"] for k in res["cand"]) >= 2
    kw, src, tgt = polish_ref.sparse_scene(pkg)
    hyp = polish_ref.hypotheses(O, src, tgt, kw)
    res = polish_ref.polish(O, src, tgt, hyp["Rt"], kw["tau"], 0, 64, 16)
    stops = [k["stop"] for k in res["cand"]]
    print("sparse:", hyp["t_eff"], len(res["cand"]), [(k["score0"], k["iters"], k["stop"]) for k in res["cand"]])
    assert res["status"] == 0 and 0 < len(res["cand"]) < hyp["t_eff"] <= 40 < 64
    assert "declined" in stops and "fixed" in stops
    assert all(k["iters"] == 0 and k["score0"] < 3 for k in res["cand"] if k["stop"] == "declined")
