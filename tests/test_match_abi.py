"""CPU suite: the surface of sc_match (include/saccot.h) — exports, the Python mirror, the struct layout — and the numpy
restatement of the canonical matcher (tests/match_ref.py) that the GPU tests compare against, checked here against an
independent fp64 brute force, on its tie rule, and against a stored fixture.  No compute call is made: there is no GPU here."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import match_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_match_default_params", "sc_match_device", "sc_match", "sc_register_features")


def test_match_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "saccot.h")).read()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    assert L.sc_version() >> 16 == 0 and L.sc_version() & 0xFFFF >= 10
    assert "#define SC_VERSION_MINOR 10" in header
    for method in ("match", "match_device", "register_features"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.api.SC_MATCH_MUTUAL == 1 and "#define SC_MATCH_MUTUAL 1u" in header


def test_match_params_layout_and_defaults(pkg):
    exe = os.path.join(ROOT, "tests", ".abi_probe_match")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("%zu %zu %zu %zu %zu", sizeof(sc_match_params), '
           'offsetof(sc_match_params, dim), offsetof(sc_match_params, knn), offsetof(sc_match_params, ratio), sizeof(sc_params));return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    try:
        size, o_dim, o_knn, o_ratio, size_p = (int(x) for x in subprocess.check_output([exe]).decode().split())
    finally:
        os.remove(exe)
    M = pkg.api.ScMatchParams
    assert (size, o_dim, o_knn, o_ratio) == (C.sizeof(M), M.dim.offset, M.knn.offset, M.ratio.offset)
    assert size_p == 64  # sc_params did not move
    m = M()
    assert pkg.load_library().sc_match_default_params(C.byref(m)) == 0  # (host only: no GPU needed)
    assert (m.size, m.dim, m.knn, m.flags, m.ratio, list(m.reserved)) == (C.sizeof(M), 0, 1, 0, 0.0, [0, 0, 0])
    assert pkg.load_library().sc_match_default_params(None) == -1
    mm = pkg.api.make_match_params(33, mutual=True, ratio=0.5)
    assert (mm.size, mm.dim, mm.knn, mm.flags, mm.ratio) == (C.sizeof(M), 33, 1, 1, 0.5)


# ---- the restatement against an independent fp64 brute force -----------------------------------------------------
# Inputs on which fp32 rounding cannot change anything: integer-valued descriptors below 2^10 whose every partial sum stays
# below 2^24 — D * max|a - b|^2 <= 2^24 — so every fp32 operation of the chain is exact: values below 2^9 at D = 64
# (64 * 511^2 < 2^24), values below 2^10 at D = 16 (16 * 1023^2 < 2^24).
def _integer_case(seed, ns, nt, D, top):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, top, (ns, D)).astype(np.float32)
    b = rng.integers(0, top, (nt, D)).astype(np.float32)
    near = rng.permutation(nt)[: ns // 2]
    b[near] = a[: len(near)] + rng.integers(-2, 3, (len(near), D)).astype(np.float32)  # counterparts: the ratio test keeps some
    b = np.clip(b, 0, top - 1)
    b[nt - 1] = b[0]                                                                   # ... and ties
    a[ns - 1] = a[0]
    return a, b


def _brute64(a, b, knn=1, mutual=False, ratio=0.0):
    d = ((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    assert d.max() < 2 ** 24
    corr, d2 = [], []
    for i in range(a.shape[0]):
        js = sorted(range(b.shape[0]), key=lambda j: (d[i, j], j))
        if mutual or ratio > 0:
            j = js[0]
            ok = True
            if mutual:
                ok = min(range(a.shape[0]), key=lambda ii: (d[ii, j], ii)) == i
            if ratio > 0 and len(js) > 1:
                ok = ok and d[i, j] < float(np.float32(ratio)) ** 2 * d[i, js[1]]
            js = [j] if ok else []
        for j in js[:knn]:
            corr.append((i, j)); d2.append(d[i, j])
    return np.array(corr, np.int32).reshape(-1, 2), np.array(d2, np.float32)


@pytest.mark.parametrize("ns,nt,D,top", [(40, 55, 64, 512), (33, 20, 16, 1024), (5, 3, 7, 1024), (6, 1, 64, 512)])
def test_restatement_equals_fp64_brute_force(ns, nt, D, top):
    a, b = _integer_case(100 + D + ns, ns, nt, D, top)
    # ratio 0.5 and 0.25: r2 = 1/4, 1/16 and r2 * acc2 are exact in fp32 as in fp64
    for kw in (dict(knn=1), dict(knn=4), dict(knn=2), dict(knn=1, mutual=True), dict(knn=1, ratio=0.5), dict(knn=1, ratio=0.25),
               dict(knn=1, mutual=True, ratio=0.5)):
        got_c, got_d = match_ref.match(a, b, **kw)
        exp_c, exp_d = _brute64(a, b, **kw)
        assert np.array_equal(got_c, exp_c), kw
        assert got_d.tobytes() == exp_d.tobytes(), kw
        assert got_c.dtype == np.int32 and got_d.dtype == np.float32
        if kw.get("ratio"):
            assert 0 < len(got_c) < ns or nt == 1, (kw, len(got_c))  # (the test discriminates)
    if nt == 1:
        assert len(match_ref.match(a, b, ratio=0.5)[0]) == ns  # one target: nothing to compare with, kept


def test_restatement_tie_rule():
    rng = np.random.default_rng(7)
    a = rng.standard_normal((6, 9)).astype(np.float32)
    b = np.concatenate([a[[2, 2, 0, 0, 0]], rng.standard_normal((3, 9)).astype(np.float32) + 10])
    a[5] = a[0]                     # source rows 0 and 5 equal; target rows 2, 3, 4 equal them, rows 0 and 1 equal source row 2
    corr, d2 = match_ref.match(a, b, knn=3)
    assert corr[:3].tolist() == [[0, 2], [0, 3], [0, 4]] and d2[:3].tolist() == [0, 0, 0]
    assert corr[6:8].tolist() == [[2, 0], [2, 1]]
    corr, _ = match_ref.match(a, b, mutual=True)
    pairs = set(map(tuple, corr.tolist()))
    assert (0, 2) in pairs and (5, 2) not in pairs and (2, 0) in pairs  # the lower source index holds the mutual pair
    # all-equal descriptors: every distance 0, the answer is pure index order
    z = np.ones((4, 5), np.float32)
    corr, d2 = match_ref.match(z, np.ones((7, 5), np.float32), knn=4)
    assert corr.tolist() == [[i, j] for i in range(4) for j in range(4)] and not d2.any()
    assert match_ref.match(z, np.ones((7, 5), np.float32), mutual=True)[0].tolist() == [[0, 0]]
    # the distance itself: symmetric bit for bit, and +inf is an ordinary value
    big = (rng.standard_normal((3, 4)) * 2.0 ** 63).astype(np.float32)
    d = match_ref.distances(big, -big)
    assert np.isinf(d).any() and d.tobytes() == match_ref.distances(-big, big).T.copy().tobytes()


def test_make_feature_scene(pkg):
    S = pkg.synth
    cfg = S.CONFIGS["C0"]
    a = S.make_feature_scene(cfg, 300, 32, 1.0)
    b = S.make_feature_scene(cfg, 300, 32, 1.0, cfg.seed)
    for k in ("src_pts", "tgt_pts", "fsrc", "ftgt", "truth"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert a.src_pts.shape == (500, 3) and a.tgt_pts.shape == (800, 3) and a.fsrc.shape == (500, 32) and a.ftgt.shape == (800, 32)
    assert all(getattr(a, k).dtype == np.float32 for k in ("src_pts", "tgt_pts", "fsrc", "ftgt")) and a.truth.dtype == np.int32
    base = S.make_scene(cfg.n, 2 * cfg.rho, cfg.L, cfg.tau, cfg.seed)
    own = a.truth >= 0
    assert np.array_equal(own, base.inlier) and own.sum() == 300 and len(set(a.truth[own].tolist())) == 300
    assert a.src_pts.tobytes() == base.src.tobytes()
    assert a.tgt_pts[a.truth[own]].tobytes() == base.tgt[own].tobytes()  # a true counterpart follows the motion (make_scene's noise)
    # a counterpart's descriptor is its source's plus unit-ish noise; anything else is independent of it
    d_own = np.linalg.norm(a.ftgt[a.truth[own]] - a.fsrc[own], axis=1)
    assert 3.0 < d_own.mean() < 8.0  # sd * sqrt(32) = 5.7
    c = S.make_feature_scene(cfg, 300, 32, 1.0, cfg.seed + 1)
    assert c.ftgt.tobytes() != a.ftgt.tobytes() and c.truth.tobytes() != a.truth.tobytes()
    d = S.make_feature_scene(cfg, 300, 33, 1.0)
    assert d.fsrc.shape == (500, 33) and np.array_equal(d.truth, a.truth)


def test_make_scene_still_produces_the_golden_bits(pkg):
    g = np.load(os.path.join(ROOT, "tests", "golden", "c0.npz"))
    cfg, scene = pkg.synth.make_config_scene("C0")
    assert scene.src.tobytes() == np.ascontiguousarray(g["src"]).tobytes()
    assert scene.tgt.tobytes() == np.ascontiguousarray(g["tgt"]).tobytes()


def test_match_micro_fixture(pkg):
    """tests/golden/match_micro.npz: the stored inputs are what the generator beside it makes, and the restatement still returns
    the stored outputs (64 x 80 x 33, planted ties) — the restatement cannot drift without this test noticing."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "match_micro.npz"))
    spec = importlib.util.spec_from_file_location("make_match_micro", os.path.join(ROOT, "tests", "golden", "make_match_micro.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    a, b = gen.inputs()
    assert a.tobytes() == g["fsrc"].tobytes() and b.tobytes() == g["ftgt"].tobytes() and a.shape == (64, 33) and b.shape == (80, 33)
    for name, kw in gen.MODES.items():
        corr, d2 = match_ref.match(g["fsrc"], g["ftgt"], **kw)
        assert np.array_equal(corr, g["corr_" + name]) and d2.tobytes() == g["d2_" + name].tobytes(), name
    k1, k4 = g["corr_k1"], g["corr_k4"]
    assert k1[9].tolist() == [9, 3] and k4[36:39, 1].tolist() == [3, 11, 70]  # the tripled target row: lowest index first
    assert g["d2_k1"][60] == 0 and k1[60].tolist() == [60, 20]
    assert np.array_equal(k4[::4], k1) and len(g["corr_mutual"]) < 64 and len(g["corr_ratio"]) < 64
