"""CPU suite: the surface of sc_register_batch (include/saccot.h) — the two exports, the Python mirror, the struct layout, the
argument checks that need no GPU — and the restatement the GPU tests compare against (tests/batch_ref.py), checked here on the
goldens.  No compute call reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import batch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_register_batch", "sc_register_batch_device")
SC_EINVAL = -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_batch_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("register_batch", "register_batch_device"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.ScBatchResult is pkg.api.ScBatchResult and pkg.BATCH_RESULT_DTYPE is pkg.api.BATCH_RESULT_DTYPE
    assert pkg.SC_BATCH_MAX_N == 512 and re.search(r"^#define SC_BATCH_MAX_N 512u\b", header, flags=re.M)


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_BATCH 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_batch_result_layout(pkg):
    exe = os.path.join(ROOT, "tests", ".abi_probe_batch")
    fields = ("Rt", "status", "n", "edges", "tri_kept", "tri_total", "best_rank", "best_count")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("%zu %zu %zu ' + "%zu " * len(fields) + '", '
           'sizeof(sc_batch_result), sizeof(sc_params), sizeof(sc_stats), '
           + ", ".join(f"offsetof(sc_batch_result, {f})" for f in fields) + ');return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    finally:
        os.remove(exe)
    B, dt = pkg.api.ScBatchResult, pkg.api.BATCH_RESULT_DTYPE
    assert got[0] == 80 == C.sizeof(B) == dt.itemsize == batch_ref.RESULT_DTYPE.itemsize
    assert got[1] == C.sizeof(pkg.ScParams) == 64 and got[2] == C.sizeof(pkg.ScStats)  # neither moved
    assert got[3:] == [getattr(B, f).offset for f in fields] == [dt.fields[f][1] for f in fields] == [0, 48, 52, 56, 60, 64, 72, 76]
    assert dt == batch_ref.RESULT_DTYPE


def test_null_arguments_are_refused_without_a_gpu(pkg):
    L = pkg.load_library()
    p = pkg.make_params()
    off = (C.c_uint32 * 2)(0, 8)
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on a NULL before it looks at anything else
    f32 = (C.c_float * 24)(); mask = (C.c_uint8 * 8)()
    # (a context cannot exist here — sc_create fails without a GPU — so the NULL context is what is tried; the GPU suite tries the rest)
    assert L.sc_register_batch(None, f32, f32, off, 1, C.byref(p), fake, mask) == SC_EINVAL
    assert L.sc_register_batch_device(None, fake, fake, off, 1, C.byref(p), fake, fake) == SC_EINVAL
    assert L.sc_register_batch(None, None, None, None, 0, None, None, None) == SC_EINVAL
    assert L.sc_register_batch_device(None, None, None, None, 0, None, None, None) == SC_EINVAL


def test_the_reference_reproduces_the_goldens(O):
    gold = [np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) for name in ("micro64", "c0")]
    problems = [(g["src"], g["tgt"]) for g in gold]
    for b, g in enumerate(gold):  # one sc_params serves a batch: each golden's own T in turn, the golden checked under its own
        sigma, t_cmp, tau, min_len = (float(x) for x in g["params"])
        kw = dict(sigma=sigma, t_cmp=t_cmp, tau=tau, min_len=min_len, max_triangles=int(g["T"]), rank_mode=0)
        recs, masks = batch_ref.batch(O, problems, kw)
        r = recs[b]
        assert r["status"] == 0 and r["n"] == len(g["src"]) and r["edges"] == int(g["edges"]) and r["tri_total"] == int(g["tri_total"])
        assert r["tri_kept"] == len(g["tri"]) and r["best_rank"] == int(g["best_rank"]) and r["best_count"] == int(g["best_count"])
        assert r["Rt"].tobytes() == np.concatenate([g["R"].ravel(), g["t"]]).astype(np.float32).tobytes()
        assert np.array_equal(masks[b], g["mask"])
        assert all(recs[k]["status"] == 0 for k in range(2))


def test_the_reference_zeroes_a_non_finite_problem_and_keeps_its_neighbours(pkg, O):
    s, t = batch_ref.scene(pkg, 64, .3)
    bad = t.copy(); bad[5, 1] = np.nan
    kw = dict(batch_ref.KW, max_triangles=200)
    recs, masks = batch_ref.batch(O, [(s, t), (s, bad), (s, t)], kw)
    assert list(recs["status"]) == [0, SC_EINVAL, 0] and recs[0].tobytes() == recs[2].tobytes()
    z = recs[1]
    assert z["Rt"].tobytes() == batch_ref.IDENT.tobytes() and z["n"] == 64 and not masks[1].any()
    assert (z["edges"], z["tri_kept"], z["tri_total"], z["best_rank"], z["best_count"]) == (0, 0, 0, 0, 0)


def test_the_scenes_of_the_gpu_tests_are_what_they_are_used_for(pkg, O):
    """The table of the GPU tests' scenes: every one stays under the triangle cap, scene (3, 1.0) is a natural SC_ENOHYP, and
    the exact scene's keys are all equal."""
    kw = dict(batch_ref.KW, max_triangles=200)
    recs, _ = batch_ref.batch(O, batch_ref.mixed(pkg), kw)
    table = [(int(r["edges"]), int(r["tri_total"])) for r in recs]
    print(table)
    assert table == [(1, 0), (5, 2), (202, 334), (216, 287), (212, 422), (779, 2884), (2836, 14813), (8532, 64962), (12579, 198326)]
    assert max(t for _, t in table) <= batch_ref.TRI_CAP
    assert recs[0]["status"] == batch_ref.SC_ENOHYP and all(r["status"] == 0 for r in recs[1:])
    src, tgt = batch_ref.exact_scene()
    r, m = batch_ref.one(O, src, tgt, dict(batch_ref.KW, max_triangles=1001))
    S, bits, deg = O.compat(src, tgt, 0.05, 0.9, 0.05, 0.05)
    tri, key, total = O.triangles(S, bits, deg, 1001, 0)
    print(int(r["edges"]), int(r["tri_total"]), int(r["best_rank"]), int(r["best_count"]), tri[-1])
    assert (int(r["edges"]), int(r["tri_total"]), int(r["tri_kept"]), int(r["best_rank"]), int(r["best_count"])) == (780, 9880, 1001, 0, 40)
    assert tuple(int(x) for x in tri[-1]) == (1, 9, 31)  # the last of the 1001 kept: (i, j, k) alone orders equal keys
    assert len(set(key.tolist())) == 1 and key[0] == np.float32(3.0).view(np.uint32)
