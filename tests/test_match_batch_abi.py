"""CPU suite: the surface of sc_match_batch / sc_register_batch_features (include/saccot.h) — the four exports, the Python mirror,
the argument checks that need no GPU, the host-only offset checks under the address and undefined-behaviour sanitizers (a
stand-alone program) — and the composed reference the GPU tests compare against (tests/match_batch_ref.py), checked here on the
scenes those tests use.  No compute call reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import batch_ref
import match_batch_ref as M
import match_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_match_batch", "sc_match_batch_device", "sc_register_batch_features", "sc_register_batch_features_device")
SC_EINVAL = -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_the_four_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("match_batch", "match_batch_device", "register_batch_features", "register_batch_features_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.SC_MATCH_BATCH_MAX_N == pkg.api.SC_MATCH_BATCH_MAX_N == 4096
    assert re.search(r"^#define SC_MATCH_BATCH_MAX_N 4096u\b", header, flags=re.M)


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_MATCH_BATCH 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10
    assert C.sizeof(pkg.ScParams) == 64


def test_null_arguments_are_refused_without_a_gpu(pkg):
    L = pkg.load_library()
    p, mp = pkg.make_params(), pkg.api.make_match_params(4)
    off = (C.c_uint32 * 2)(0, 2)
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on a NULL before it looks at anything else
    f32 = (C.c_float * 8)(); i32 = (C.c_int32 * 4)(); cnt = (C.c_uint32 * 2)(); mask = (C.c_uint8 * 2)()
    # (a context cannot exist here — sc_create fails without a GPU — so the NULL context is what is tried; the GPU suite tries the rest)
    assert L.sc_match_batch(None, f32, off, f32, off, 1, C.byref(mp), i32, f32, cnt) == SC_EINVAL
    assert L.sc_match_batch_device(None, fake, off, fake, off, 1, C.byref(mp), fake, fake, fake) == SC_EINVAL
    assert L.sc_register_batch_features(None, f32, f32, off, f32, f32, off, 1, C.byref(mp), C.byref(p), fake, i32, f32, cnt, mask) == SC_EINVAL
    assert L.sc_register_batch_features_device(None, fake, fake, off, fake, fake, off, 1, C.byref(mp), C.byref(p), fake, fake, fake, fake,
                                               fake) == SC_EINVAL
    assert L.sc_match_batch(None, None, None, None, None, 0, None, None, None, None) == SC_EINVAL
    assert L.sc_register_batch_features(None, None, None, None, None, None, None, 0, None, None, None, None, None, None, None) == SC_EINVAL


def test_the_host_offset_checks_under_the_sanitizers(tmp_path):
    """Decreasing offsets, empty problems, a side above SC_MATCH_BATCH_MAX_N, the features entries' slot bound, total_s * knn at and
    above 2^31, and the tile map: tests/native/match_batch_check_main.cpp, a program of its own built with
    -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "match_batch_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "match_batch_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


def test_the_scenes_of_the_gpu_tests_are_what_they_are_used_for(O):
    """Conditions on the shared scenes (tests/match_batch_ref.py), on the composed reference:
    every gathered problem holds at most batch_ref.TRI_CAP triangles (both match modes the GPU test runs);
    with SC_MATCH_MUTUAL the scenes hold a problem with n_b < 3, one with n_b == 3 and a natural SC_ENOHYP with n_b >= 3, and every
    other problem is SC_OK with a rotation within 0.5 degrees of the generator's; with knn = 2 every match is followed by a random
    second neighbour, and every scene of 16 keypoints or more with inliers is still SC_OK within 0.5 degrees;
    the tie scene has equal distances in a row."""
    scenes = M.feature_scenes()
    table = {}
    for tag, mkw in (("mutual", dict(knn=1, mutual=True)), ("knn2", dict(knn=2))):
        table[tag] = [M.features_one(O, s[0], s[1], s[2], s[3], mkw, M.KW) for s in scenes]
        for r, s in zip(table[tag], scenes):
            print(tag, len(s[0]), r["n"], int(r["rec"]["status"]), int(r["rec"]["tri_total"]), int(r["rec"]["best_count"]))
            assert int(r["rec"]["tri_total"]) <= batch_ref.TRI_CAP and r["flag"] == 0
    mut = table["mutual"]
    short = [k for k, r in enumerate(mut) if r["n"] < 3]
    three = [k for k, r in enumerate(mut) if r["n"] == 3]
    natural = [k for k, r in enumerate(mut) if r["n"] >= 3 and r["rec"]["status"] == M.SC_ENOHYP]
    assert short and three and natural
    assert all(mut[k]["rec"]["status"] == M.SC_ENOHYP and mut[k]["rec"]["n"] == mut[k]["n"] for k in short)
    for k, (r, s) in enumerate(zip(mut, scenes)):
        if k in short or k in natural:
            continue
        err = M.rotation_error_deg(r["rec"]["Rt"][:9], s[4])
        print("mutual", len(s[0]), "rotation error", err)
        assert r["rec"]["status"] == M.SC_OK and err < 0.5, (k, err)
    for (n, rho, _), r, s in zip(M.FEATURE_SCENES, table["knn2"], scenes):
        assert r["n"] == 2 * n  # (nt_b == ns_b >= 2: every row has two neighbours)
        if n >= 16 and rho > 0:
            assert r["rec"]["status"] == M.SC_OK and M.rotation_error_deg(r["rec"]["Rt"][:9], s[4]) < 0.5, n
    for a, b in M.tie_descriptors():
        acc = match_ref.distances(a, b)
        assert any(len(set(row.tolist())) < len(row) for row in acc)      # equal distances in a row ...
        assert any(len(set(col.tolist())) < len(col) for col in acc.T)    # ... and in a column (the mutual test's order)
        assert (np.sort(acc, axis=1)[:, 0] == np.sort(acc, axis=1)[:, 1]).any()  # ... among them a row whose MINIMUM is tied


def test_the_reference_flags_a_non_finite_problem_only(O):
    a, b = M.mixed_descriptors(17)[4]
    bad = a.copy(); bad[-1, -1] = np.nan
    assert M.match_one(bad, b)[2:] == (0, 1) and M.match_one(a, b)[3] == 0
    s = M.feature_scenes()[3]
    fb = s[1].copy(); fb[0, 0] = np.inf
    r = M.features_one(O, s[0], fb, s[2], s[3], dict(knn=1, mutual=True), M.KW)
    assert r["rec"]["status"] == SC_EINVAL and r["rec"]["n"] == 0 and r["rec"]["Rt"].tobytes() == batch_ref.IDENT.tobytes()
