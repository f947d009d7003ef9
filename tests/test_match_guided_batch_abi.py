"""CPU suite: the surface of sc_match_guided_batch (include/saccot.h) — the six exports, the Python mirror, the feature macro and the
flag, the argument checks that need no GPU (the host-only rules also under the sanitizers, in a program of their own) — and the numpy
restatement of its semantics (tests/match_guided_batch_ref.py) that the GPU tests compare against, checked on itself: with an open
gate it is match_batch_ref, and the shared batch and table hold what the GPU tests use them for.  No compute call reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import match_batch_ref as MB
import match_guided_batch_ref as GB
import match_guided_ref as MG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_match_guided_batch_device", "sc_match_guided_batch", "sc_register_guided_batch_features_device",
         "sc_match_guided_pairs_device", "sc_match_guided_pairs", "sc_register_guided_pairs_features_device")
METHODS = ("match_guided_batch", "match_guided_batch_device", "register_guided_batch_features_device", "match_guided_pairs",
           "match_guided_pairs_device", "register_guided_pairs_features_device")
SC_OK, SC_EINVAL = 0, -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_the_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) in (15, 16, 18, 19)
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in METHODS:
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.SC_GUIDE_POSE_STATUS == pkg.api.SC_GUIDE_POSE_STATUS == 1
    for word in ("host forms of the two features entries", "one pose shared by all problems", "several poses per problem", "an instances\n * form",
                 "batch and pairs forms (entries of their own: sc_match_guided_batch"):
        assert word in header  # what is not here is said, and where the forms the frame entry lacks are


def test_the_minor_version_stays_and_the_macros_are_there(pkg, tmp_path):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_MATCH_GUIDED_BATCH 1\b", header, flags=re.M)
    assert re.search(r"^#define SC_GUIDE_POSE_STATUS 1u\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10
    exe = str(tmp_path / "probe")
    src = ('#include <stdio.h>\n#include "saccot.h"\nint main(void){printf("%u %u %u", (unsigned)SC_HAS_MATCH_GUIDED_BATCH, '
           '(unsigned)SC_GUIDE_POSE_STATUS, (unsigned)sizeof(sc_guide_params));return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    assert subprocess.check_output([exe]).decode().split() == ["1", "1", "32"]


def test_every_entry_is_refused_without_a_context(pkg):
    L = pkg.load_library()
    mp, gp, p = pkg.api.make_match_params(8), pkg.make_guide_params(0.1), pkg.make_params()
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on the NULL context before it looks at anything else
    f32, i32 = C.cast(fake, C.POINTER(C.c_float)), C.cast(fake, C.POINTER(C.c_int32))
    u32 = C.cast(fake, C.POINTER(C.c_uint32))
    m, g, q = C.byref(mp), C.byref(gp), C.byref(p)
    assert L.sc_match_guided_batch_device(None, fake, fake, u32, fake, fake, u32, 1, m, g, fake, 48, fake, fake, fake, fake) == SC_EINVAL
    assert L.sc_match_guided_batch(None, f32, f32, u32, f32, f32, u32, 1, m, g, fake, 48, i32, f32, f32, u32) == SC_EINVAL
    assert L.sc_register_guided_batch_features_device(None, fake, fake, u32, fake, fake, u32, 1, m, g, fake, 48, q, fake, fake, fake, fake,
                                                      fake, fake) == SC_EINVAL
    assert L.sc_match_guided_pairs_device(None, fake, fake, u32, 1, u32, 1, m, g, fake, 48, fake, fake, fake, fake) == SC_EINVAL
    assert L.sc_match_guided_pairs(None, f32, f32, u32, 1, u32, 1, m, g, fake, 48, i32, f32, f32, u32) == SC_EINVAL
    assert L.sc_register_guided_pairs_features_device(None, fake, fake, u32, 1, u32, 1, m, g, fake, 48, q, fake, fake, fake, fake, fake,
                                                      fake) == SC_EINVAL
    for name in NAMES:  # ... and with nothing at all
        f = getattr(L, name)
        assert f(*[0 if t is C.c_uint32 else None for t in f.argtypes]) == SC_EINVAL


def test_the_host_checks_under_the_sanitizers(tmp_path):
    """Every refusal of the guide block with the one flag allowed (flags 1 and 2), and pose strides 44 / 48 / 50 / 52 with and
    without the flag: tests/native/match_guided_batch_check_main.cpp, a program of its own built with
    -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "match_guided_batch_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "match_guided_batch_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


# ---- the restatement checked on itself -----------------------------------------------------------------------------------------------
def test_an_open_gate_is_the_plain_batch_matcher():
    batch = GB.mixed_batch(33)
    for kw in MG.MODES:
        corr, d2, g2, count = GB.match_batch(batch, MG.GATE_ALL, **kw)
        knn = kw.get("knn", 1)
        so, _ = batch.offsets()
        for b, sc in enumerate(batch.scenes):
            ec, ed, n, flag = MB.match_one(sc.fsrc, sc.ftgt, **kw)
            lo = int(so[b]) * knn
            assert count[b].tolist() == [n, flag] and (n > 0 or sc.fsrc.shape[0] * sc.ftgt.shape[0] == 0), (b, kw)
            assert corr[lo: lo + n].tobytes() == ec.tobytes() and d2[lo: lo + n].tobytes() == ed.tobytes(), (b, kw)
            hi = int(so[b + 1]) * knn
            assert (corr[lo + n: hi] == GB.FILL_I).all() and (d2[lo + n: hi] == np.float32(GB.FILL_F)).all() and \
                (g2[lo + n: hi] == np.float32(GB.FILL_F)).all(), (b, kw)


def test_the_shared_batch_has_what_the_gpu_tests_use_it_for():
    batch = GB.shared_batch(33)
    assert [(len(s.fsrc), len(s.ftgt)) for s in batch.scenes[:GB.MIXED_N]] == list(GB.MIXED)
    # a problem with rows that have no, one and several admissible candidates
    per_row = batch.problem(4, MG.GATE).adm.sum(axis=1)
    print("admissible per row: none", int((per_row == 0).sum()), "one", int((per_row == 1).sum()), "more", int((per_row >= 2).sum()))
    assert (per_row == 0).any() and (per_row == 1).any() and (per_row >= 2).any()
    # a problem in which whole 64 x 64 tiles, and whole 64-row tiles, admit nothing
    tiles = batch.problem(GB.SKIP_AT, MG.GATE).adm.reshape(6, 64, 3, 64).any(axis=(1, 3))
    assert tiles.tolist() == [[False, True, False]] * 2 + [[True, False, False]] * 2 + [[False, False, False]] * 2
    # a problem under a hostile finite pose: nothing admissible at any gate, and no flag
    hostile = batch.scenes[GB.HOSTILE_AT]
    assert np.isfinite(hostile.Rt).all()
    for gate in (MG.GATE, MG.GATE_ALL):
        assert not np.isfinite(batch.problem(GB.HOSTILE_AT, gate).g2).any()
        assert GB.one(batch, GB.HOSTILE_AT, gate, knn=4)[3:] == (0, 0)
    # the poses differ from problem to problem: a kernel that reads problem 0's pose for all fails
    poses = batch.poses()
    assert len({p.tobytes() for p in poses}) == len(poses)
    wrong = GB.match_batch(batch, MG.GATE, poses=np.tile(poses[0], (len(batch), 1)))
    right = GB.match_batch(batch, MG.GATE)
    assert wrong[3][0].tolist() == right[3][0].tolist() and wrong[3][3].tolist() != right[3][3].tolist()
    # the gates: nothing / everything
    assert not GB.match_batch(batch, MG.GATE_NOTHING, knn=4)[3].any()
    # a flagged and a skipped problem: (0, 1) and (0, 0), and the neighbours' bytes are what they were
    bad = GB.with_scene(batch, 3, fsrc=np.where(np.arange(33) == 5, np.nan, batch.scenes[3].fsrc).astype(np.float32))
    flagged = GB.match_batch(bad, MG.GATE)
    assert flagged[3][3].tolist() == [0, 1] and np.array_equal(np.delete(flagged[3], 3, 0), np.delete(right[3], 3, 0))
    status = np.zeros(len(batch), np.int32); status[3] = GB.SC_ENOHYP
    skipped = GB.match_batch(batch, MG.GATE, statuses=status)
    assert skipped[3][3].tolist() == [0, 0]
    so, _ = batch.offsets()
    lo, hi = int(so[3]), int(so[4])
    for a in (0, 1, 2):
        assert (np.delete(skipped[a], np.s_[lo:hi], 0) == np.delete(right[a], np.s_[lo:hi], 0)).all()
    assert (skipped[0][lo:hi] == GB.FILL_I).all() and (skipped[1][lo:hi] == np.float32(GB.FILL_F)).all()  # the slot is untouched


def test_the_pose_records():
    batch = GB.mixed_batch(1)
    for dt in (GB.POSE64, GB.POSE80):
        rec = batch.poses(dt, statuses=[0, -5, 0, -1, 0])
        assert rec.dtype.itemsize in (64, 80) and rec.dtype.fields["status"][1] == 48 and rec.dtype.fields["Rt"][1] == 0
        assert rec["Rt"].tobytes() == batch.poses().tobytes() and rec["status"].tolist() == [0, -5, 0, -1, 0]


def test_the_pairs_table_has_what_the_gpu_tests_use_it_for():
    tab = GB.table()
    pairs = GB.PAIRS.tolist()
    assert [len(p) for p, _ in tab["sets"]] == list(GB.PAIR_SIZES) and len(tab["poses"]) == len(pairs)
    assert pairs.count([0, 1]) == 2 and [2, 2] in pairs and sum(1 for a, b in pairs if b == 3) == 2
    assert len({p.tobytes() for p in tab["poses"]}) == len(pairs)  # the repeated pair has two poses: its two slots differ
    eb = GB.expand(tab, GB.PAIRS, tab["poses"])
    count = GB.match_batch(eb, MG.GATE)[3]
    print(count.tolist())
    assert (count[:, 0] > 0).all() and not count[:, 1].any() and count[0].tolist() != count[2].tolist()
    per_row = eb.problem(1, MG.GATE).adm.sum(axis=1)
    assert (per_row == 0).any() and (per_row == 1).any() and (per_row >= 2).any()
