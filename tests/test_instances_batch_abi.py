"""CPU suite: the surface of sc_register_instances_batch (include/saccot.h) — the three exports, the Python mirror, the argument checks
that need no GPU — and the scenes of tests/test_gpu_instances_batch.py, checked here on the reference alone
(tests/instances_batch_ref.py).  No compute call reaches a GPU."""
import ctypes as C
import os
import re

import numpy as np

import batch_ref
import instances_batch_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_register_instances_batch", "sc_register_instances_batch_device", "sc_register_instances_batch_features_device")
SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("register_instances_batch_raw", "register_instances_batch", "register_instances_batch_device",
                   "register_instances_batch_features_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.SC_INSTANCES_BATCH_MAX == 16 and re.search(r"^#define SC_INSTANCES_BATCH_MAX 16u\b", header, flags=re.M)


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_INSTANCES_BATCH 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_arguments_are_refused_without_a_gpu(pkg):
    """(a context cannot exist here — sc_create fails without a GPU — so the NULL context is what is tried; the GPU suite tries the rest
    with a context and reads sc_last_error)"""
    L = pkg.load_library()
    p = pkg.make_params()
    bad = pkg.make_params(tau=-1.0)
    mp = pkg.api.make_match_params(4)
    off = (C.c_uint32 * 2)(0, 8)
    fake = C.c_void_p(64)  # never dereferenced
    f32 = (C.c_float * 24)(); lab = (C.c_int32 * 8)(); nf = (C.c_uint32 * 1)()
    for k, q in ((4, p), (0, p), (17, p), (4, bad)):
        assert L.sc_register_instances_batch(None, f32, f32, off, 1, C.byref(q), k, 4, fake, lab, nf) == SC_EINVAL
        assert L.sc_register_instances_batch_device(None, fake, fake, off, 1, C.byref(q), k, 4, fake, fake, fake) == SC_EINVAL
        assert L.sc_register_instances_batch_features_device(None, fake, fake, off, fake, fake, off, 1, C.byref(mp), C.byref(q), k, 4, fake,
                                                             fake, fake, fake, fake, fake) == SC_EINVAL
    assert L.sc_register_instances_batch(None, None, None, None, 0, None, 4, 4, None, None, None) == SC_EINVAL
    assert L.sc_register_instances_batch_device(None, None, None, None, 0, None, 4, 4, None, None, None) == SC_EINVAL
    assert L.sc_register_instances_batch_features_device(None, None, None, None, None, None, None, 0, None, None, 4, 4, None, None, None,
                                                         None, None, None) == SC_EINVAL


# ---- the scenes are what the GPU tests use them for: asserted on the reference alone -----------------------------------------------
_REF = {}


def _ref(pkg, O, T, rank_mode=0, mode=0, min_score=4):
    """-> ([(planes, label, nfound)], [info]) of the shared scenes, once per session and parameter set"""
    key = (T, rank_mode, mode, min_score)
    if key not in _REF:
        kw = dict(IR.KW, max_triangles=T, rank_mode=rank_mode)
        infos = [dict() for _ in IR.SCENES]
        _REF[key] = ([IR.one(O, s, t, kw, mode, 4, min_score, infos[b]) for b, (s, t) in enumerate(IR.scenes(pkg))], infos)
    return _REF[key]


def test_two_motions_at_T_2000(pkg, O):
    out, infos = _ref(pkg, O, 2000)
    found = [int(f) for _, _, f in out]
    scores = [tuple(int(x) for x in planes["best_count"][:f]) for planes, _, f in out]
    totals = [int(planes[0]["tri_total"]) for planes, _, _ in out]
    print(found, scores, totals)
    assert found == [0, 0, 2, 2, 2, 2, 2, 2]
    assert scores[2:] == [(18, 12), (18, 12), (18, 13), (39, 25), (59, 39), (89, 59)]
    for (planes, label, f), (n, _) in zip(out, IR.SCENES):
        if n <= 4:  # no triangle
            assert planes[0]["status"] == SC_ENOHYP and (planes["status"] == SC_ENOHYP).all() and (label == -1).all()
        else:
            assert planes[0]["status"] == SC_OK and list(planes["status"]) == [SC_OK, SC_OK, SC_ENOHYP, SC_ENOHYP]
            assert [int((label == k).sum()) for k in range(2)] == [int(planes[k]["best_count"]) for k in range(2)]  # inlier count
            e = planes[2]
            assert e["Rt"].tobytes() == batch_ref.IDENT.tobytes() and e["best_rank"] == 0 and e["best_count"] == 0
            assert all(e[f] == planes[0][f] for f in ("n", "edges", "tri_kept", "tri_total"))
    # which problems select: more triangles than T from n = 128 on, fewer below; no workgroup runs long
    assert all(t > 2000 for t in totals[5:]) and all(t <= 2000 for t in totals[:5])
    assert (min(totals[5:]), max(totals)) == (3730, 57738) and max(totals) <= batch_ref.TRI_CAP


def test_more_motions_at_T_50(pkg, O):
    out, _ = _ref(pkg, O, 50)
    found = {n: int(f) for (_, _, f), (n, _) in zip(out, IR.SCENES)}
    print(found)
    assert found[128] == 3 and found[512] == 3 and found[257] == 4


def test_a_motion_outside_the_top_T_is_not_found(pkg, O):
    """Degree ranking, MSE score, T = 2000, n = 128: none of the second motion's triangles made the top T, so it is NOT found — what the
    contract says (sc_peel: not "run the path again on the rest")."""
    s, t = IR.scene(pkg, 128, .5)
    planes, label, found = IR.one(O, s, t, dict(IR.KW, max_triangles=2000, rank_mode=1), 1, 4, 4 * 256)
    print(found, planes["best_count"])
    assert found == 1 and planes[1]["status"] == SC_ENOHYP


def test_a_rounds_winner_has_a_claimed_vertex(pkg, O):
    """A kept triangle stays a hypothesis when its vertices are claimed: at T = 50 with weight ranking the scenes of 128, 257 and 512
    correspondences each have a later round's winner with a claimed vertex, so the GPU suite's mixed batch covers the case."""
    hits = []
    for T in (2000, 50):
        for rank_mode in (0, 1):
            _, infos = _ref(pkg, O, T, rank_mode)
            hits += [(T, rank_mode, n) for inf, (n, _) in zip(infos, IR.SCENES) if inf.get("claimed_vertex")]
    print(hits)
    assert (50, 0, 128) in hits and (50, 0, 257) in hits and (50, 0, 512) in hits  # weight ranking, T = 50: cases of the GPU suite


def test_empty_planes_and_min_score_on_the_reference(pkg, O):
    s, t = IR.scene(pkg, 64, .5)
    kw = dict(IR.KW, max_triangles=2000)
    planes, label, found = IR.one(O, s, t, kw, 0, 4, 10 ** 6)
    assert found == 0 and (label == -1).all() and planes[0]["status"] == SC_OK and planes[0]["best_count"] == 18
    assert list(planes["status"][1:]) == [SC_ENOHYP] * 3
    bad = t.copy(); bad[5, 1] = np.nan
    planes, label, found = IR.one(O, s, bad, kw, 0, 4, 4)
    assert found == 0 and (label == -1).all() and (planes["status"] == SC_EINVAL).all() and (planes["n"] == 64).all()
