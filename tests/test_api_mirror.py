"""CPU suite: sac-cot_amd/api.py against what it mirrors.  The prototype table against the two headers (parameter count, pointer or
scalar, width and signedness, result type), the five records' numpy dtypes against their structures, and the marshalling helpers at
the smallest shapes where they can go wrong.  Nothing here creates a context or reaches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
RESULTS = {"int": C.c_int, "void": None, "const char*": C.c_char_p}


def _prototypes():
    """name -> (result type, [parameter, ...]) for every `sc_*` function the two headers declare"""
    text = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("saccot.h", "saccot_debug.h"))
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for res, name, params in re.findall(r"^(int|void|const char\*)\s+(sc_\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        assert name not in out, f"{name} is declared twice"
        params = [" ".join(p.split()) for p in params.split(",")]  # (no parameter holds a comma: none is a function pointer)
        out[name] = (res, [] if params == ["void"] else params)
    return out


def _is_pointer(t):
    return t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def _scalar_kind(t):
    """(bytes, signed, floating) of a ctypes scalar"""
    return C.sizeof(t), t(-1).value < 0, isinstance(t(0).value, float)


def test_exports_follow_from_the_table_and_the_library_has_them_all(pkg):
    api = pkg.api
    assert api.EXPORTS == list(api._PROTOTYPES) and len(set(api.EXPORTS)) == len(api.EXPORTS) >= 95  # (95 when the table came)
    written = re.findall(r'^    "(sc_\w+)": ', open(api.__file__).read(), flags=re.M)
    assert written == api.EXPORTS  # (a name written twice in the literal would drop out of the dict without a word)
    L = pkg.load_library()
    for name in api.EXPORTS:
        fn = getattr(L, name)
        assert fn.argtypes is not None, f"{name} has no argtypes"
        assert len(fn.argtypes) > 0 or name == "sc_version", f"{name} has an empty argument list"


def test_the_table_mirrors_the_headers_parameter_by_parameter(pkg):
    L, protos = pkg.load_library(), _prototypes()
    for name in pkg.api.EXPORTS:
        assert name in protos, f"{name} is in no header"
        res, params = protos[name]
        fn = getattr(L, name)
        assert len(params) == len(fn.argtypes), f"{name}: {len(params)} parameters declared, {len(fn.argtypes)} mirrored"
        for k, (param, t) in enumerate(zip(params, fn.argtypes)):
            where = f"{name}, parameter {k} ({param})"
            if "*" in param or "[" in param:
                assert _is_pointer(t), where + f" is a pointer, mirrored by {t}"
            else:
                ctype = param.replace("const ", "").split(" ")[0]
                assert ctype in SCALARS, where + ": a scalar type this test does not know"
                assert not _is_pointer(t) and _scalar_kind(t) == _scalar_kind(SCALARS[ctype]), where + f" is mirrored by {t}"
        assert fn.restype is RESULTS[res], f"{name} returns {res}, mirrored by {fn.restype}"
    char_p = {n for n in pkg.api.EXPORTS if getattr(L, n).restype is C.c_char_p}
    void = {n for n in pkg.api.EXPORTS if getattr(L, n).restype is None}
    assert char_p == {"sc_strerror", "sc_last_error", "sc_multi_last_error"}
    assert void == {n for n in pkg.api.EXPORTS if protos[n][0] == "void"} == {"sc_default_params", "sc_destroy", "sc_destroy_multi"}


def test_every_function_of_the_headers_is_in_the_table(pkg):
    assert sorted(_prototypes()) == sorted(pkg.api.EXPORTS)


@pytest.mark.parametrize("struct, dtype", [("ScBatchResult", "BATCH_RESULT_DTYPE"), ("ScPolishCand", "POLISH_CAND_DTYPE"),
                                           ("ScPolishBatchResult", "POLISH_BATCH_RESULT_DTYPE"),
                                           ("ScPoseInfoResult", "POSE_INFO_RESULT_DTYPE"), ("ScAssignResult", "ASSIGN_RESULT_DTYPE")])
def test_a_record_has_one_definition(pkg, struct, dtype):
    S, D = getattr(pkg.api, struct), getattr(pkg.api, dtype)
    assert np.dtype(S) == D and D.itemsize == C.sizeof(S)
    assert list(D.names) == [f[0] for f in S._fields_]
    assert [D.fields[f[0]][1] for f in S._fields_] == [getattr(S, f[0]).offset for f in S._fields_]


def test_pose_records_of_plain_arrays(pkg):
    rec = pkg.Registrar._pose_records
    one = np.arange(12, dtype=np.float64)
    for pose, k in ((one, 1), (np.stack([one, one + 1, one + 2]), 3), (list(range(12)), 1)):
        got, stride = rec(pose)
        assert got.dtype == np.float32 and got.shape == (k, 12) and got.flags.c_contiguous and stride == 48
        assert np.array_equal(got[0], np.arange(12, dtype=np.float32))
    strided = np.zeros((3, 24))[:, ::2]  # (a view that is not contiguous comes out contiguous)
    assert rec(strided)[0].flags.c_contiguous
    assert rec(np.stack([one, one]), 2)[0].shape == (2, 12)
    with pytest.raises(ValueError):
        rec(np.stack([one, one]), 3)


@pytest.mark.parametrize("dtype", ["BATCH_RESULT_DTYPE", "POLISH_BATCH_RESULT_DTYPE"])
def test_pose_records_of_records(pkg, dtype):
    D = getattr(pkg.api, dtype)
    planes = np.zeros((2, 3), D)
    planes["status"] = np.arange(6).reshape(2, 3)
    got, stride = pkg.Registrar._pose_records(planes)
    assert got.dtype == D and got.shape == (6,) and stride == D.itemsize and list(got["status"]) == list(range(6))
    assert pkg.Registrar._pose_records(planes, 6)[1] == D.itemsize
    with pytest.raises(ValueError):
        pkg.Registrar._pose_records(planes, 2)


def test_frame_sel(pkg):
    sel = pkg.api._frame_sel
    assert sel("who", None, np.uint8, 5) is None
    for dtype in (np.uint8, np.int32):
        got = sel("who", [1, 0, 1, 1, 0], dtype, 5)
        assert got.dtype == dtype and got.flags.c_contiguous and list(got) == [1, 0, 1, 1, 0]
    assert sel("who", np.ones((2, 3), np.int64), np.uint8, 6).dtype == np.uint8  # (size counts, as before: not the shape)
    for wrong in (4, 6, 0):
        with pytest.raises(ValueError, match="who: sel holds one entry per correspondence of the frame"):
            sel("who", np.zeros(5, np.uint8), np.uint8, wrong)
    assert sel("who", [], np.uint8, 0).size == 0


def test_offsets(pkg):
    u32c, total = pkg.api._u32c, pkg.api._total
    for given, nb, tot in (([], 0, 0), ([0], 0, 0), ([0, 3, 3, 7], 3, 7), (np.array([0, 2], np.int64), 1, 2)):
        off, got_nb = u32c(given)
        assert off.dtype == np.uint32 and off.flags.c_contiguous and list(off) == list(given)
        assert (got_nb, total(off)) == (nb, tot)
    off = np.array([0, 4], np.uint32)
    assert u32c(off)[0] is off  # (an array that is already right is passed on, not copied)


def test_n_points(pkg):
    a = np.zeros((5, 3), np.float32)
    assert pkg.api._n_points(a, pkg.SC_AOS) == 5 and pkg.api._n_points(a.T, pkg.SC_SOA) == 5
    assert pkg.api._n_points(np.zeros((3, 3)), pkg.SC_SOA) == 3


def test_frame_outputs(pkg):
    api = pkg.api
    for ns, knn, cap in ((0, 1, 1), (0, 4, 1), (1, 4, 4), (3, 0, 3), (5, 2, 10)):  # (knn 0 is the library's to refuse: room as for 1)
        out, count = api._frame_out(ns, knn, g2=True, label=True, mask=True)
        assert list(out) == ["corr", "d2", "g2", "label", "mask"] and isinstance(count, C.c_uint32) and count.value == 0
        assert out["corr"].shape == (cap, 2) and [out[k].shape for k in ("d2", "g2", "label", "mask")] == [(cap,)] * 4
        assert [out[k].dtype for k in out] == [np.int32, np.float32, np.float32, np.int32, np.uint8]
    out, count = api._frame_out(1, 4)
    assert list(out) == ["corr", "d2"]
    assert list(api._frame_out(1, 4, label=True)[0]) == ["corr", "d2", "label"]
    out["corr"][:] = np.arange(8).reshape(4, 2); out["d2"][:] = [4, 3, 2, 1]
    count.value = 3
    cut = api._frame_cut(out, count)
    assert list(cut) == ["n", "corr", "d2"] and cut["n"] == 3
    assert np.array_equal(cut["corr"], [[0, 1], [2, 3], [4, 5]]) and list(cut["d2"]) == [4, 3, 2]
    assert not np.shares_memory(cut["corr"], out["corr"]) and not np.shares_memory(cut["d2"], out["d2"])  # copies
    count.value = 0
    assert api._frame_cut(out, count)["corr"].shape == (0, 2)


def test_slot_outputs(pkg):
    api = pkg.api
    o = api._slot_out(0, 0)  # no slot, no problem: still room for one of each, and g2 is NULL for the library
    assert list(o) == ["corr", "d2", "g2", "count"] and o["g2"] is None and api._p(o["g2"]) is None
    assert o["corr"].shape == (1, 2) and o["d2"].shape == (1,) and o["count"].shape == (1, 2)
    assert [o[k].dtype for k in ("corr", "d2", "count")] == [np.int32, np.float32, np.uint32]
    corr, d2, g2, count = api._slot_cut(o, 0, 0, "corr", "d2", "g2", "count")
    assert corr.shape == (0, 2) and d2.shape == (0,) and g2 is None and count.shape == (0, 2)
    o = api._slot_out(7, 3, g2=True, registered=True)
    assert list(o) == ["corr", "d2", "g2", "count", "res", "mask"]
    assert o["g2"].shape == (7,) and o["g2"].dtype == np.float32 and o["mask"].shape == (7,) and o["mask"].dtype == np.uint8
    assert o["res"].shape == (3,) and o["res"].dtype == api.BATCH_RESULT_DTYPE and o["count"].shape == (3, 2)
    res, corr, d2, count, mask = api._slot_cut(o, 5, 2, "res", "corr", "d2", "count", "mask")
    assert (len(res), len(corr), len(d2), len(count), len(mask)) == (2, 5, 5, 2, 5)
    assert all(np.shares_memory(a, o[k]) for a, k in ((res, "res"), (corr, "corr"), (d2, "d2"), (count, "count"), (mask, "mask")))  # views
    o = api._slot_out(0, 0, registered=True)
    assert o["res"].shape == (1,) and o["mask"].shape == (1,)


def test_pointers_take_their_type_from_the_array(pkg):
    api = pkg.api
    assert api._p(None) is None and api._vp(None) is None
    for dtype, ctype in ((np.float32, C.c_float), (np.uint8, C.c_uint8), (np.int32, C.c_int32), (np.uint32, C.c_uint32),
                         (np.uint64, C.c_uint64)):
        a = np.arange(6, dtype=dtype).reshape(3, 2)
        ptr = api._p(a)
        assert isinstance(ptr, C.POINTER(ctype)) and C.addressof(ptr.contents) == a.ctypes.data and ptr[5] == 5
    rec = np.zeros(2, api.ASSIGN_RESULT_DTYPE)
    assert isinstance(api._vp(rec), C.c_void_p) and api._vp(rec).value == rec.ctypes.data
    with pytest.raises(KeyError):
        api._p(np.zeros(3))  # float64: no parameter of the ABI takes it typed


def test_result_and_sized(pkg):
    api = pkg.api
    R, t, st = api._motion_out()
    assert R.shape == (9,) and t.shape == (3,) and R.dtype == t.dtype == np.float32 and st.size == C.sizeof(api.ScStats)
    got = api._result(-5, R, t, st, mask=np.ones(2, np.uint8), n=2)
    assert list(got) == ["status", "R", "t", "mask", "n", "stats"] and got["R"].shape == (3, 3) and got["status"] == -5
    assert np.shares_memory(got["R"], R) and "size" not in got["stats"] and got["stats"]["n"] == 0
    for make, cls in ((api.make_params, api.ScParams), (api.make_polish_params, api.ScPolishParams),
                      (api.make_settle_params, api.ScSettleParams), (api.make_assign_params, api.ScAssignParams)):
        assert make().size == C.sizeof(cls)
    assert api.make_match_params(32, mutual=True).flags == api.SC_MATCH_MUTUAL and api.make_guide_params(0.5).gate == 0.5
