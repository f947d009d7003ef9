"""CPU suite: the surface of sc_polish_batch (include/saccot.h) — the three exports, the Python mirror, the struct layout, the argument
checks that need no GPU — and the numpy restatement of its semantics (tests/polish_batch_ref.py) that the GPU tests compare against,
checked here for what its scenes are used for.  No compute call reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import batch_ref
import polish_batch_ref as PB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_polish_batch", "sc_polish_batch_device", "sc_polish_batch_slots_device")
SC_OK, SC_EINVAL = 0, -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_polish_batch_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("polish_batch_raw", "polish_batch_device", "polish_batch_slots_device", "register_batch_polished"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.ScPolishBatchResult is pkg.api.ScPolishBatchResult


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_POLISH_BATCH 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_polish_batch_result_layout(pkg):
    exe = os.path.join(ROOT, "tests", ".abi_probe_polish_batch")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d", '
           'sizeof(sc_polish_batch_result), offsetof(sc_polish_batch_result, Rt), offsetof(sc_polish_batch_result, status), '
           'offsetof(sc_polish_batch_result, score0), offsetof(sc_polish_batch_result, score), offsetof(sc_polish_batch_result, iters), '
           'offsetof(sc_polish_batch_result, stop), sizeof(sc_batch_result), sizeof(sc_polish_params), '
           'SC_POLISH_STOP_FIXED, SC_POLISH_STOP_DECLINED, SC_POLISH_STOP_MAX_ITER);return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    finally:
        os.remove(exe)
    K = pkg.api.ScPolishBatchResult
    assert got[:7] == [64, K.Rt.offset, K.status.offset, K.score0.offset, K.score.offset, K.iters.offset, K.stop.offset] and C.sizeof(K) == 64
    assert got[1:7] == [0, 48, 52, 56, 60, 62]
    assert got[7:9] == [C.sizeof(pkg.ScBatchResult), C.sizeof(pkg.ScPolishParams)]  # neither moved
    assert got[9:] == [pkg.api.SC_POLISH_STOP_FIXED, pkg.api.SC_POLISH_STOP_DECLINED, pkg.api.SC_POLISH_STOP_MAX_ITER] == \
           [PB.STOP_FIXED, PB.STOP_DECLINED, PB.STOP_MAX_ITER]
    for dt in (pkg.api.POLISH_BATCH_RESULT_DTYPE, PB.RESULT_DTYPE):
        assert dt.itemsize == 64 and [dt.fields[k][1] for k in ("Rt", "status", "score0", "score", "iters", "stop")] == [0, 48, 52, 56, 60, 62]


def test_null_arguments_and_bad_params_are_refused_without_a_gpu(pkg):
    L = pkg.load_library()
    p = pkg.make_params(**PB.kw_of(0.02))
    q = pkg.make_polish_params(candidates=1)
    off = np.array([0, 8], np.uint32)
    u32p = C.POINTER(C.c_uint32)
    o = off.ctypes.data_as(u32p)
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on the NULL context before it looks at anything else
    f32 = np.zeros((8, 3), np.float32).ctypes.data_as(C.POINTER(C.c_float))
    m8 = np.zeros(8, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    # (a context cannot exist here — sc_create fails without a GPU — so the NULL arguments and the bad parameter blocks are tried
    # with a NULL context; the GPU suite repeats them on a real one, where sc_last_error names the reason)
    assert L.sc_polish_batch(None, f32, f32, o, 1, C.byref(p), C.byref(q), fake, fake, m8) == SC_EINVAL
    assert L.sc_polish_batch(None, None, f32, o, 1, C.byref(p), C.byref(q), fake, fake, m8) == SC_EINVAL
    assert L.sc_polish_batch(None, f32, f32, o, 1, C.byref(p), None, fake, fake, m8) == SC_EINVAL
    assert L.sc_polish_batch_device(None, fake, fake, o, 1, C.byref(p), C.byref(q), fake, fake, fake) == SC_EINVAL
    assert L.sc_polish_batch_device(None, fake, fake, None, 1, C.byref(p), C.byref(q), fake, fake, None) == SC_EINVAL
    assert L.sc_polish_batch_slots_device(None, fake, o, fake, o, 1, 1, C.byref(p), C.byref(q), fake, fake, fake, fake, fake) == SC_EINVAL
    assert L.sc_polish_batch_slots_device(None, None, o, fake, None, 1, 1, None, None, fake, fake, fake, fake, fake) == SC_EINVAL
    for bad in (pkg.make_polish_params(candidates=8), pkg.make_polish_params(candidates=1, max_iter=0),
                pkg.make_polish_params(candidates=1, max_iter=65), pkg.make_polish_params(candidates=1, flags=1)):
        assert L.sc_polish_batch(None, f32, f32, o, 1, C.byref(p), C.byref(bad), fake, fake, m8) == SC_EINVAL
        assert L.sc_polish_batch_device(None, fake, fake, o, 1, C.byref(p), C.byref(bad), fake, fake, fake) == SC_EINVAL


# ---- the scenes are what the GPU tests use them for: asserted on the reference alone -----------------------------------------
def test_the_mixed_scene_stops_every_way_iterates_and_moves_the_count(pkg, O):
    problems = PB.mixed(pkg)
    assert [len(s) for s, _ in problems] == [3, 4, 63, 64, 65, 128, 129, 257, 512, 512]
    recs, _ = batch_ref.batch(O, problems, PB.kw_of(0.02))
    assert int(recs["tri_total"].max()) <= batch_ref.TRI_CAP  # no workgroup of sc_register_batch runs long
    two, _ = PB.batch(O, problems, recs, 0.02, 0, 2)
    full, masks = PB.batch(O, problems, recs, 0.02, 0, 16)
    print([tuple(int(o[f]) for f in PB.FIELDS) for o in two])
    print([tuple(int(o[f]) for f in PB.FIELDS) for o in full])
    ok = full["status"] == SC_OK
    assert PB.STOP_MAX_ITER in two["stop"][ok] and PB.STOP_FIXED in full["stop"][ok]
    assert PB.STOP_MAX_ITER not in full["stop"]  # 16 refits reach every fixed point
    assert {int(x) for x in np.concatenate([two["stop"], full["stop"]])} == {PB.STOP_FIXED, PB.STOP_DECLINED, PB.STOP_MAX_ITER}
    assert int(full["iters"].max()) >= 3
    assert (full["score"][ok] < full["score0"][ok]).any() and (full["score"][ok] > full["score0"][ok]).any()
    assert np.array_equal(full["score0"][ok], recs["best_count"][ok])  # the input pose's score IS the batch record's count
    for b in np.flatnonzero(ok):
        assert int(masks[b].sum()) == int(full["score"][b])  # inlier-count mode
    for b in np.flatnonzero(~ok):  # passed through
        assert full["status"][b] == recs["status"][b] and full["Rt"][b].tobytes() == batch_ref.IDENT.tobytes() and not masks[b].any()
        assert (int(full["score0"][b]), int(full["score"][b]), int(full["iters"][b]), int(full["stop"][b])) == (0, 0, 0, PB.STOP_DECLINED)
    # the truncated squared residual is raised at both scales
    for tau in PB.TAUS:
        r1, _ = batch_ref.batch(O, problems, PB.kw_of(tau), 1)
        o1, _ = PB.batch(O, problems, r1, tau, 1, 16)
        good = o1["status"] == SC_OK
        assert (o1["score"][good] >= o1["score0"][good]).all() and (o1["score"][good] > o1["score0"][good]).any(), tau


def test_the_sparse_problem_has_a_winner_whose_first_refit_is_declined(pkg, O):
    kw, src, tgt = PB.sparse(pkg)
    assert 3 <= len(src) <= 128 and kw["tau"] == 0.001
    rec, mask = batch_ref.one(O, src, tgt, kw)
    assert rec["status"] == SC_OK and 0 < rec["best_count"] < 3 and rec["tri_total"] <= batch_ref.TRI_CAP
    out, omask = PB.one(O, src, tgt, rec, kw["tau"], 0, 16)
    assert (int(out["status"]), int(out["iters"]), int(out["stop"])) == (SC_OK, 0, PB.STOP_DECLINED)
    assert out["Rt"].tobytes() == rec["Rt"].tobytes() and out["score"] == out["score0"] == rec["best_count"]
    assert np.array_equal(omask, mask)


def test_status_rules_of_the_reference(pkg, O):
    s, t = batch_ref.scene(pkg, 64, .3)
    rec, _ = batch_ref.one(O, s, t, PB.kw_of(0.05))
    assert rec["status"] == SC_OK
    nan_t = t.copy(); nan_t[5, 1] = np.nan
    bad_rt = rec.copy(); bad_rt["Rt"][7] = np.nan
    nohyp = rec.copy(); nohyp["status"] = PB.SC_ENOHYP
    for (a, b, r), want in (((s, nan_t, rec), SC_EINVAL), ((s, t, bad_rt), SC_EINVAL), ((s, t, nohyp), PB.SC_ENOHYP)):
        out, m = PB.one(O, a, b, r, 0.05)
        assert (int(out["status"]), int(out["score0"]), int(out["score"]), int(out["iters"]), int(out["stop"])) == (want, 0, 0, 0, PB.STOP_DECLINED)
        assert out["Rt"].tobytes() == batch_ref.IDENT.tobytes() and not m.any() and len(m) == 64
