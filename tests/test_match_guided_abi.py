"""CPU suite: the surface of sc_match_guided (include/saccot.h) — the four exports, the Python mirror, the layout of sc_guide_params,
the default parameters, the argument checks that need no GPU (also under the sanitizers, in a program of their own) — and the numpy
restatement of its semantics (tests/match_guided_ref.py) that the GPU tests compare against, checked on itself: with a gate that admits
everything it is match_ref, and the shared scene has what the GPU tests use it for.  No compute call reaches a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import match_guided_ref as MG
import match_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_guide_default_params", "sc_match_guided_device", "sc_match_guided", "sc_register_guided_features")
SC_OK, SC_EINVAL = 0, -1


def _header():
    return open(os.path.join(ROOT, "include", "saccot.h")).read()


def test_guided_entries_are_exported_declared_and_mirrored(pkg):
    L = pkg.load_library()
    header = _header()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    code = re.sub(r"/\*.*?\*/", "", header + open(os.path.join(ROOT, "include", "saccot_debug.h")).read(), flags=re.S)
    assert sorted(pkg.api.EXPORTS) == sorted(set(re.findall(r"\b(sc_[a-z_]+)\s*\(", code)))
    for method in ("match_guided", "match_guided_device", "register_guided_features"):
        assert callable(getattr(pkg.Registrar, method))
    assert pkg.ScGuideParams is pkg.api.ScGuideParams and callable(pkg.make_guide_params)
    for word in ("batch and pairs forms", "several poses per call", "a gate on anything but the point residual", "soft weighting by g2"):
        assert word in header  # what is not here is said


def test_the_minor_version_stays_and_the_feature_macro_is_there(pkg):
    header = _header()
    assert "#define SC_VERSION_MINOR 10" in header and re.search(r"^#define SC_HAS_MATCH_GUIDED 1\b", header, flags=re.M)
    assert pkg.load_library().sc_version() == 10


def test_guide_params_layout(pkg):
    exe = os.path.join(ROOT, "tests", ".abi_probe_match_guided")
    P = "sc_guide_params"
    fields = [f"sizeof({P})"] + [f"offsetof({P}, {f})" for f in ("size", "layout", "gate", "flags", "reserved")]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "saccot.h"\nint main(void){printf("' + "%zu " * len(fields) + '%u", '
           + ", ".join(fields) + ", (unsigned)SC_HAS_MATCH_GUIDED);return 0;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)  # (the header is still plain C99)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    finally:
        os.remove(exe)
    K = pkg.api.ScGuideParams
    assert got == [32, 0, 4, 8, 12, 16, 1]
    assert got[:6] == [C.sizeof(K), K.size.offset, K.layout.offset, K.gate.offset, K.flags.offset, K.reserved.offset]


def test_default_params(pkg):
    L = pkg.load_library()
    gp = pkg.ScGuideParams(1, 2, 3.0, 4)
    gp.reserved[3] = 9
    assert L.sc_guide_default_params(C.byref(gp)) == SC_OK
    assert bytes(gp) == (32).to_bytes(4, "little") + bytes(28)  # size set, SC_AOS, gate 0: the caller sets it
    assert L.sc_guide_default_params(None) == SC_EINVAL
    q = pkg.make_guide_params(0.25, pkg.SC_SOA)
    assert (q.size, q.layout, q.gate, q.flags, list(q.reserved)) == (32, 1, 0.25, 0, [0, 0, 0, 0])


def test_every_entry_is_refused_without_a_context(pkg):
    L = pkg.load_library()
    mp, gp, p = pkg.api.make_match_params(8), pkg.make_guide_params(0.1), pkg.make_params()
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused on the NULL context before it looks at anything else
    f32 = C.cast(fake, C.POINTER(C.c_float))
    i32, u32, u8 = C.cast(fake, C.POINTER(C.c_int32)), C.cast(fake, C.POINTER(C.c_uint32)), C.cast(fake, C.POINTER(C.c_uint8))
    assert L.sc_match_guided_device(None, fake, fake, 4, fake, fake, 4, C.byref(mp), C.byref(gp), fake, fake, fake, fake, fake) == SC_EINVAL
    assert L.sc_match_guided_device(None, None, None, 0, None, None, 0, None, None, None, None, None, None, None) == SC_EINVAL
    n = C.c_uint32(7)
    assert L.sc_match_guided(None, f32, f32, 4, f32, f32, 4, C.byref(mp), C.byref(gp), f32, i32, f32, f32, C.byref(n)) == SC_EINVAL
    assert n.value == 0
    assert L.sc_match_guided(None, None, None, 0, None, None, 0, None, None, None, None, None, None, None) == SC_EINVAL
    n = C.c_uint32(7)
    assert L.sc_register_guided_features(None, f32, f32, 4, f32, f32, 4, C.byref(mp), C.byref(gp), f32, C.byref(p), f32, f32, i32, f32, f32,
                                         C.byref(n), u8, None) == SC_EINVAL
    assert n.value == 0
    assert L.sc_register_guided_features(None, None, None, 0, None, None, 0, None, None, None, None, None, None, None, None, None, None,
                                         None, None) == SC_EINVAL
    del u32


def test_the_host_checks_under_the_sanitizers(tmp_path):
    """Every refusal of sc_guide_params and the boundary values of the gate (0, negative, NaN, inf, the smallest subnormal, FLT_MAX):
    tests/native/match_guided_check_main.cpp, a program of its own built with -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "match_guided_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "native", "match_guided_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all passed" in out.stdout and "runtime error" not in out.stderr


# ---- the restatement checked on itself -----------------------------------------------------------------------------------------------
def test_a_gate_that_admits_everything_is_the_plain_matcher():
    for ns, nt, D in ((300, 333, 33), (3, 5, 1), (1, 1, 2), (65, 63, 4)):
        sc = MG.shared_scene(ns, nt, D)
        prob = MG.Problem(*sc.args(), MG.GATE_ALL)
        assert prob.adm.all() and np.isfinite(MG.gate2_of(MG.GATE_ALL))
        for kw in MG.MODES:
            c, d, g = prob.match(**kw)
            ec, ed = match_ref.match(sc.fsrc, sc.ftgt, **kw)
            assert c.tobytes() == ec.tobytes() and d.tobytes() == ed.tobytes() and len(g) == len(c), (ns, nt, D, kw)


def test_the_shared_scene_has_what_the_gpu_tests_use_it_for():
    sc = MG.shared_scene(300, 333, 33)
    prob = MG.Problem(*sc.args(), MG.GATE)
    per_row = prob.adm.sum(axis=1)
    print("admissible per row: none", int((per_row == 0).sum()), "one", int((per_row == 1).sum()), "more", int((per_row >= 2).sum()))
    assert (per_row == 0).any() and (per_row == 1).any() and (per_row >= 2).any()
    assert not MG.Problem(*sc.args(), MG.GATE_NOTHING).adm.any()
    for kw in MG.MODES:
        c, d, g = prob.match(**kw)
        bc, bd = match_ref.match(sc.fsrc, sc.ftgt, **kw)
        inside = prob.adm[bc[:, 0], bc[:, 1]]
        print(kw, "guided", len(c), "blind", len(bc), "blind filtered by the gate", int(inside.sum()))
        # guided matching is neither the blind match nor the blind match filtered afterwards: rows are re-assigned
        assert c.tobytes() != bc.tobytes() and c.tobytes() != bc[inside].tobytes(), kw
        assert len(c) > inside.sum() and (g < MG.gate2_of(MG.GATE)).all() and prob.adm[c[:, 0], c[:, 1]].all(), kw
        assert g.tobytes() == prob.g2[c[:, 0], c[:, 1]].tobytes() and d.tobytes() == prob.acc[c[:, 0], c[:, 1]].tobytes()


def test_the_residual_of_all_pairs_is_the_pairwise_one():
    sc = MG.shared_scene(65, 63, 1)
    g2 = MG.gate_residuals(sc.Rt, sc.src_pts, sc.tgt_pts)
    import assign_ref as AR
    for i in (0, 17, 64):
        assert g2[i].tobytes() == AR.resid2(sc.Rt, np.repeat(sc.src_pts[i:i + 1], 63, axis=0), sc.tgt_pts).tobytes()
    hostile = MG.gate_residuals(AR.hostile(), sc.src_pts, sc.tgt_pts)
    assert not np.isfinite(hostile).any() and not MG.admissible(hostile, MG.GATE_ALL).any() and np.isfinite(AR.hostile()).all()
