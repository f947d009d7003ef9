"""CPU suite: the surface of sc_match_pairs / sc_register_pairs_features / sc_polish_pairs_slots_device (include/saccot.h) — the six
exports, the Python mirror, the argument checks that need no GPU, sc_pairs_layout against a Python restatement, the host-only checks
of the table and the list under the address and undefined-behaviour sanitizers (a stand-alone program) — and the composed reference
the GPU tests compare against (tests/pairs_ref.py), checked here on the table and the list those tests use.  No compute call reaches
a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_ref
import match_ref
import pairs_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_pairs_layout", "sc_match_pairs", "sc_match_pairs_device", "sc_register_pairs_features", "sc_register_pairs_features_device",
         "sc_polish_pairs_slots_device")
SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_the_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("pairs_layout", "match_pairs", "match_pairs_device", "register_pairs_features", "register_pairs_features_device",
                   "polish_pairs_slots_device"):
        assert callable(getattr(pkg.Registrar, method))


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_PAIRS 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_null_arguments_are_refused_without_a_gpu(pkg):
    L = pkg.load_library()
    p, mp, q = pkg.make_params(), pkg.api.make_match_params(4), pkg.make_polish_params(candidates=1)
    off = (C.c_uint32 * 2)(0, 2); prs = (C.c_uint32 * 2)(0, 0); slot = (C.c_uint32 * 2)()
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on a NULL before it looks at anything else
    f32 = (C.c_float * 8)(); i32 = (C.c_int32 * 4)(); cnt = (C.c_uint32 * 2)(); mask = (C.c_uint8 * 2)()
    # (a context cannot exist here — sc_create fails without a GPU — so the NULL context is what is tried; the GPU suite tries the rest)
    assert L.sc_match_pairs(None, f32, off, 1, prs, 1, C.byref(mp), i32, f32, cnt) == SC_EINVAL
    assert L.sc_match_pairs_device(None, fake, off, 1, prs, 1, C.byref(mp), fake, fake, fake) == SC_EINVAL
    assert L.sc_register_pairs_features(None, f32, f32, off, 1, prs, 1, C.byref(mp), C.byref(p), fake, i32, f32, cnt, mask) == SC_EINVAL
    assert L.sc_register_pairs_features_device(None, fake, fake, off, 1, prs, 1, C.byref(mp), C.byref(p), fake, fake, fake, fake, fake) == SC_EINVAL
    assert L.sc_polish_pairs_slots_device(None, fake, off, 1, prs, 1, 1, C.byref(p), C.byref(q), fake, fake, fake, fake, fake) == SC_EINVAL
    assert L.sc_match_pairs(None, None, None, 0, None, 0, None, None, None, None) == SC_EINVAL
    # sc_pairs_layout has no context: its three pointers
    assert L.sc_pairs_layout(off, 1, prs, 1, 1, slot) == SC_OK and list(slot) == [0, 2]
    assert L.sc_pairs_layout(None, 1, prs, 1, 1, slot) == SC_EINVAL
    assert L.sc_pairs_layout(off, 1, None, 1, 1, slot) == SC_EINVAL
    assert L.sc_pairs_layout(off, 1, prs, 1, 1, None) == SC_EINVAL


def test_pairs_layout_equals_the_restatement(pkg):
    layout = pkg.Registrar.pairs_layout
    # sets: 0: 5 rows, 1: 0 rows (referenced by nobody), 2: 64, 3: 1, 4: 257
    off = np.array([0, 5, 5, 69, 70, 327], np.uint32)
    lists = ([(4, 3), (2, 2), (4, 3), (3, 0), (2, 0), (0, 4)],  # a repeated pair, a self pair, descending order
             [(0, 0)], [(3, 4), (3, 4), (3, 4)])
    for pairs in lists:
        for knn in (1, 4):
            got = layout(off, pairs, knn)
            exp = P.slots(off, pairs, knn)
            print(pairs, knn, got.tolist())
            assert got.dtype == np.uint32 and np.array_equal(got, exp)
            sizes = [int(off[a + 1] - off[a]) for a, _ in pairs]
            assert got.tolist() == [knn * sum(sizes[:p]) for p in range(len(pairs) + 1)]
    tab = P.table()
    for knn in (1, 2, 4):
        assert np.array_equal(layout(tab["set_off"], P.PAIRS, knn), P.slots(tab["set_off"], P.PAIRS, knn))
    refused = {
        "n_sets == 0": (np.array([0], np.uint32), [(0, 0)], 1),
        "n_pairs == 0": (off, np.zeros((0, 2), np.uint32), 1),
        "set_off decreasing": (np.array([0, 5, 3, 9], np.uint32), [(2, 2)], 1),
        "a set index == n_sets": (off, [(0, 5)], 1),
        "a referenced empty source": (off, [(1, 0)], 1),
        "a referenced empty target": (off, [(0, 1)], 1),
        "a referenced set of 4097 rows": (np.array([0, 4097, 4100], np.uint32), [(1, 0)], 1),
        "knn == 0": (off, [(0, 0)], 0),
        "knn == 5": (off, [(0, 0)], 5),
        "more than 2^31 entries": (np.array([0, 4096], np.uint32), np.zeros(((1 << 17) + 1, 2), np.uint32), 4),
    }
    for what, (so, pairs, knn) in refused.items():
        with pytest.raises(pkg.SacCotError) as e:
            layout(so, pairs, knn)
        assert e.value.status == SC_EINVAL, what
    # 2^31 entries exactly, and an unreferenced set above the size limit: accepted
    assert layout(np.array([0, 4096, 9000], np.uint32), np.zeros((1 << 17, 2), np.uint32), 4)[-1] == 1 << 31


def test_the_host_checks_under_the_sanitizers(tmp_path):
    """The rules of the table and the list, the slot starts, the pairs' own bases (a shared set, a column base past 2^32) and the
    tile map: tests/native/pairs_check_main.cpp, a program of its own built with -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "pairs_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "pairs_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


def test_the_table_and_the_list_are_what_the_gpu_tests_use_them_for(O):
    """On the reference alone, with SC_MATCH_MUTUAL (what the registration tests run): a set that is the target of two pairs with
    different sources, whose column minima differ between the two; a pair with n_p < 3; a natural SC_ENOHYP; every scene's own pair
    otherwise SC_OK within 0.5 degrees of the generator; a tie pair; every gathered problem within batch_ref.TRI_CAP triangles.  And
    the list's shape: unsorted, a set that is source of several pairs and target of several others, a self pair, a repeated pair, a
    target of one row, the sizes at the tile edges."""
    tab = P.table()
    pairs = P.PAIRS.tolist()
    sizes = np.diff(tab["set_off"].astype(np.int64))
    assert {1, 2, 3, 63, 64, 65, 129, 257} <= set(sizes[np.unique(P.PAIRS)].tolist()) and tab["feat"].shape[1] == 33
    assert sizes[P.EMPTY] == 0 and P.EMPTY not in P.PAIRS
    assert pairs != sorted(pairs) and pairs != sorted(pairs, key=lambda ab: ab[1])
    assert sum(a == P.R65 for a, _ in pairs) >= 3 and sum(b == P.R65 for _, b in pairs) >= 3
    assert any(a == b for a, b in pairs) and len(set(map(tuple, pairs))) < len(pairs)
    assert any(sizes[b] == 1 for _, b in pairs)
    mkw = dict(knn=1, mutual=True)
    for tag, kw in (("tau 0.05", P.KW), ("tau 0.02", dict(P.KW, tau=0.02))):
        ref = P.features(O, tab, P.PAIRS, mkw, kw)
        for p, r in enumerate(ref):
            print(tag, p, pairs[p], r["n"], int(r["rec"]["status"]), int(r["rec"]["tri_total"]), int(r["rec"]["best_count"]))
            assert int(r["rec"]["tri_total"]) <= batch_ref.TRI_CAP and r["flag"] == 0
        short = [p for p, r in enumerate(ref) if r["n"] < 3]
        natural = [p for p, r in enumerate(ref) if r["n"] >= 3 and r["rec"]["status"] == SC_ENOHYP]
        assert short and natural
        assert all(ref[p]["rec"]["status"] == SC_ENOHYP and ref[p]["rec"]["n"] == ref[p]["n"] for p in short)
        n_ok = 0
        for p, k in P.OWN_SCENE.items():
            if p in short or p in natural:
                continue
            err = P.M.rotation_error_deg(ref[p]["rec"]["Rt"][:9], tab["R"][k])
            print(tag, "pair", p, "scene", k, "rotation error", err)
            assert ref[p]["rec"]["status"] == SC_OK and err < 0.5, (p, err)
            n_ok += 1
        assert n_ok >= 5
    # a shared target under mutual matching: two sources, and the column minima of the two pairs differ (sharing them would show)
    by_target = {}
    for a, b in pairs:
        by_target.setdefault(b, set()).add(a)
    shared = [(b, sorted(srcs)) for b, srcs in by_target.items() if len(srcs) >= 2]
    assert shared
    differ = 0
    for b, srcs in shared:
        mins = [match_ref.distances(tab["sets"][a][1], tab["sets"][b][1]).min(axis=0) for a in srcs]
        differ += any(not np.array_equal(mins[0], x) for x in mins[1:])
    assert differ >= 2
    # the tie pair: equal distances in a row and in a column, among them a tied row minimum
    acc = match_ref.distances(tab["sets"][P.TIE_A][1], tab["sets"][P.TIE_B][1])
    assert [P.TIE_A, P.TIE_B] in pairs
    assert any(len(set(row.tolist())) < len(row) for row in acc) and any(len(set(col.tolist())) < len(col) for col in acc.T)
    assert (np.sort(acc, axis=1)[:, 0] == np.sort(acc, axis=1)[:, 1]).any()


def test_the_reference_flags_every_pair_of_a_non_finite_set_and_no_other():
    tab = P.table()
    pts, feat = tab["sets"][P.R65]
    bad = feat.copy(); bad[-1, -1] = np.nan
    dirty = P.with_sets(tab, {P.R65: (pts, bad)})
    clean_ref, dirty_ref = P.match(tab, P.PAIRS, dict(knn=2)), P.match(dirty, P.PAIRS, dict(knn=2))
    for (a, b), c, d in zip(P.PAIRS.tolist(), clean_ref, dirty_ref):
        if P.R65 in (a, b):
            assert d[2:] == (0, 1)
        else:
            assert d[3] == 0 and d[2] == c[2] and d[0].tobytes() == c[0].tobytes() and d[1].tobytes() == c[1].tobytes()
