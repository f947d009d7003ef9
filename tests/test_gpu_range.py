"""GPU: the HIP path == the CPU restatement, bit for bit, at the ends of the fp32 range.

Every other GPU test feeds the library coordinates between ~0.01 and 1e4 and t_cmp between 0.45 and 0.98; check_params and
stage_inputs accept any finite coordinate, any positive finite sigma / tau, any min_len >= 0 and any 0 < t_cmp < 1.  Each case
here goes through the stage hooks — compat (bit rows, degrees, S as uint32), triangles (keys, triangles, order, total,
edges), kabsch, score (every count + key), mask — and then through register with SC_FLAG_EXACT_TOTAL, all against the
restatement (tests/test_range_oracle.py checks the restatement itself on these magnitudes, and owns the scenes and windows).

Families: a  coordinates and sigma / tau / min_len times 2^k (exact), k from -70 to 70;
          b  mixed magnitudes in one wave: a block shrunk to 2^-50 around the origin + exact duplicates of it, min_len 0 / subnormal
             (sqrt_rn_fast's slow branch next to its fast one, zero radicands, the candidate test's t < 2^-100 escape, Lc == 0);
             and 64 points at 2^62 in a unit scene;
          c  both clouds far from the origin (2^20 .. 2^24: coordinates quantised to 0.06 .. 2 — exact ties, zero lengths);
          d  x times 2^-40, z times 2^40;
          e  a few points at +-3e38 (finite inputs, non-finite differences);
          f  t_cmp, sigma, tau, min_len at the ends of what check_params accepts.
In-window metamorphic check (family a): the GPU's results at k against the GPU's at k = 0, without the oracle in the loop.
"""
import numpy as np
import pytest

from conftest import nan_equal_bits
from test_gpu_peel import _assert_rounds, _expected, _host_rounds
from test_range_oracle import (GPU_KS, UNIT, WIN_A_BITS, WIN_A_S, WIN_C1, WIN_C2, WIN_REGISTER, assert_covariant, degenerate_triangles,
                               in_window, pow2, scaled, scaled_kw, scene_big, scene_ragged, stages, translated, u32)

pytestmark = pytest.mark.gpu

T = 3000
TH = 8
F_CASES = {"tcmp38": dict(t_cmp=1e-38), "tcmp44": dict(t_cmp=1e-44),                      # sc_expf on its -87 clamp, weights next to FLT_MIN
           "tcmp1": dict(t_cmp=float(np.nextafter(np.float32(1), np.float32(0)))),          # d_thr = sigma 2^-11.5
           "sigma-30": dict(sigma=1e-30), "sigma30": dict(sigma=1e30),                      # neg_inv2sig2 = -inf / -0
           "tau-30": dict(tau=1e-30), "tau25": dict(tau=1e25),                               # tau2 0 / inf, 1 / tau^2 inf / 0
           "minlen-sub": dict(min_len=1e-42), "minlen38": dict(min_len=3e38)}


def _input(pkg, name):
    """name -> (src, tgt, kw).  Everything is made of exact operations on seeded scenes."""
    fam, *arg = name.split(":")
    src, tgt = (x.copy() for x in scene_big(pkg))
    kw = dict(UNIT)
    if fam == "a":
        if arg[0] == "ragged":
            src, tgt = scene_ragged(pkg)
        k = int(arg[1])
        return scaled(src, k), scaled(tgt, k), scaled_kw(k)
    if fam == "b" and arg[0] in ("minlen0", "minlen-sub", "deep"):
        # 2^-50: radicands 2^-109 .. 2^-98, under sqrt_rn_fast's 2^-96 switch; with unit-scale sigma every pair of the block has weight
        # exactly 1, whatever the last bit of its two lengths.  "deep": the block at 2^-58 (radicands 2^-125 .. 2^-114 and subnormal ones,
        # where the fast body alone is really wrong: its fma residuals are no longer exact) AND sigma, min_len at the block's scale, so
        # that the block's weights and its min_len decisions hang on those bits while the rest of every wave takes the fast body on
        # unit-scale lengths.  (Tried: a scratch build without the slow branch fails family a at k = -56 in S, and passes k = -48 .. -50
        # and all three blocks here.)
        sh = -58 if arg[0] == "deep" else -50
        blk = slice(512, 704)                                   # 192 consecutive correspondences: three whole waves of columns
        src[blk] = scaled(src[:192], sh); tgt[blk] = scaled(tgt[:192], sh)
        src[520:526] = 0; tgt[520:526] = 0                      # the point the block was shrunk around, six times: zero lengths
        kw["min_len"] = 1e-40 if arg[0] == "minlen-sub" else 0.0
        if arg[0] == "deep":
            kw = scaled_kw(sh, tau=kw["tau"])
    elif fam == "b":                                            # "far62"
        src[64:128] = scaled(src[64:128], 62); tgt[64:128] = scaled(tgt[64:128], 62)
    elif fam == "c":
        src, tgt = translated(src, tgt, int(arg[0]), int(arg[1]))
    elif fam == "d":
        f = np.array([pow2(-40), 1, pow2(40)], np.float32)
        src, tgt, kw = src * f, tgt * f, scaled_kw(40)
    elif fam == "e":
        big = np.float32(3e38)
        src[10] = (big, 0, 0); src[700] = (-big, big, 0.1); src[1400] = (0.2, -big, big)
        tgt[11] = (0, big, 0); tgt[700] = (big, -big, 0.3); tgt[900] = (-big, -big, -big)
    elif fam == "f":
        kw.update(F_CASES[arg[0]])
    else:
        raise KeyError(name)
    return src, tgt, kw


_REF = {}


def _ref(pkg, O, name):
    """The restatement's stages on an input, once per session."""
    if name not in _REF:
        src, tgt, kw = _input(pkg, name)
        _REF[name] = (src, tgt, kw, stages(O, src, tgt, kw, T, threads=TH))
    return _REF[name]


def _check_register(pkg, reg, src, tgt, kw, r, what, **extra):
    got = reg.register(src, tgt, flags=pkg.SC_FLAG_EXACT_TOTAL | extra.pop("flags", 0), max_triangles=T, **kw, **extra)
    st = got["stats"]
    print(what, "register: status", got["status"], "edges", st["edges"], "triangles", st["tri_total"], "kept", st["tri_kept"], "rank",
          st["best_rank"], "count", st["best_count"], "| restatement", r["rc"], r["edges"], r["tri_total"], r["t_eff"], r["best_rank"], r["best_count"])
    assert got["status"] == r["rc"], what
    assert (st["edges"], st["tri_total"], st["tri_kept"]) == (r["edges"], r["tri_total"], r["t_eff"]), what
    assert (st["best_rank"], st["best_count"]) == (r["best_rank"], r["best_count"]), what
    assert np.array_equal(got["mask"], r["mask"]), what
    assert nan_equal_bits(got["R"], r["R"]) and nan_equal_bits(got["t"], r["t"]), what
    return got


def _check_all(pkg, O, reg, name):
    """Every stage hook and the whole path on one input against the restatement -> the GPU's results (shape of stages())."""
    src, tgt, kw, ref = _ref(pkg, O, name)
    p = pkg.make_params(max_triangles=T, **kw)
    S, bits, deg = reg.compat(src, tgt, p)
    print(name, "edges", int(deg.sum()) // 2, "| restatement", int(ref["deg"].sum()) // 2, "triangles", ref["total"], "finite hypotheses",
          int(np.isfinite(ref["Rt"]).all(1).sum()), "of", len(ref["Rt"]), "best count", int(ref["cnt"].max()) if len(ref["cnt"]) else 0)
    assert np.array_equal(bits, ref["bits"]) and np.array_equal(deg, ref["deg"]), (name, "adjacency")
    assert np.array_equal(u32(S), u32(ref["S"])), (name, "S")
    tri, key, total, edges = reg.triangles(src, tgt, p)
    assert total == ref["total"] and edges == int(ref["deg"].sum()) // 2, (name, "totals")
    assert np.array_equal(key, ref["key"]) and np.array_equal(tri, ref["tri"]), (name, "ranked list")
    g = dict(S=S, bits=bits, deg=deg, tri=tri, key=key, total=total, Rt=np.zeros((0, 12), np.float32), cnt=np.zeros(0, np.uint32),
             best_key=0, mask=np.zeros(len(src), np.uint8))
    if len(ref["tri"]):
        g["Rt"] = reg.kabsch(src, tgt, p, ref["tri"])
        assert nan_equal_bits(g["Rt"], ref["Rt"]), (name, "kabsch")
        g["cnt"], g["best_key"] = reg.score(src, tgt, p, ref["Rt"])
        assert np.array_equal(g["cnt"], ref["cnt"]) and g["best_key"] == ref["best_key"], (name, "score")
        best = 0xFFFFFFFF - (ref["best_key"] & 0xFFFFFFFF) if ref["best_key"] else 0
        g["mask"] = reg.mask(src, tgt, p, ref["Rt"][best])
        with np.errstate(over="ignore", under="ignore"):
            assert np.array_equal(g["mask"], O.mask(src, tgt, ref["Rt"][best], kw["tau"])), (name, "mask")
    got = _check_register(pkg, reg, src, tgt, kw, ref["reg"], name)
    g["reg"] = dict(rc=got["status"], R=got["R"], t=got["t"], mask=got["mask"], edges=got["stats"]["edges"], tri_total=got["stats"]["tri_total"],
                    t_eff=got["stats"]["tri_kept"], best_rank=got["stats"]["best_rank"], best_count=got["stats"]["best_count"])
    return g


# ---- family a ----------------------------------------------------------------------------------------------------------------
_GPU0 = {}


@pytest.mark.parametrize("k", [0] + sorted(GPU_KS, key=lambda k: (abs(k), k)))
@pytest.mark.parametrize("which", ["big", "ragged"])
def test_uniform_power_of_two_scale(pkg, O, reg, which, k):
    """k = -48 / -47: squared lengths on both sides of sqrt_rn_fast's 2^-96 switch; k <= -56: d * d, tau2, theta2, Lc subnormal or
    zero; k >= 64: squares +inf.  Inside the windows the GPU's results are also compared with the GPU's at k = 0."""
    g = _check_all(pkg, O, reg, f"a:{which}:{k}")
    if k == 0:
        _GPU0[which] = g
        assert g["reg"]["rc"] == 0 and len(g["tri"]) == T
        return
    if which not in _GPU0:
        _GPU0[which] = _check_all(pkg, O, reg, f"a:{which}:0")
    a_s = in_window(k, WIN_A_S)
    if not a_s:     # this k's ranked list is its own: C1 / C2 were run on it above, not on k = 0's
        assert_covariant(g, _GPU0[which], k, which, a_bits=in_window(k, WIN_A_BITS), a_s=False, b=False, c1=False, c2=False, whole=False)
        return
    assert_covariant(g, _GPU0[which], k, which, a_bits=True, a_s=True, b=True, c1=in_window(k, WIN_C1), c2=in_window(k, WIN_C2),
                     whole=in_window(k, WIN_REGISTER))


# ---- families b .. f ---------------------------------------------------------------------------------------------------------
OTHER = (["b:minlen0", "b:minlen-sub", "b:deep", "b:far62", "c:20:22", "c:22:24", "c:24:20", "d", "e"] + ["f:" + c for c in F_CASES])


@pytest.mark.parametrize("name", OTHER)
def test_other_families(pkg, O, reg, name):
    """Nothing is rejected that the restatement accepts; status, graph and result are the restatement's."""
    _check_all(pkg, O, reg, name)
    if name in ("f:tau-30", "f:tau25"):           # inv_tau2 / inv_tau are inf, 0 or tiny: the truncated scores
        src, tgt, kw, ref = _ref(pkg, O, name)
        for mode in (1, 2):
            with np.errstate(over="ignore", under="ignore", divide="ignore"):
                cnt0 = O.score(src, tgt, ref["Rt"], kw["tau"], threads=TH, score_mode=mode)
                r = O.register(src, tgt, threads=TH, max_triangles=T, score_mode=mode, **kw)
            cnt, key = reg.score(src, tgt, pkg.make_params(max_triangles=T, score_mode=mode, **kw), ref["Rt"])
            print(name, "score_mode", mode, "largest score", int(cnt0.max()))
            assert np.array_equal(cnt, cnt0) and key == O.best_key(cnt0), (name, mode)
            _check_register(pkg, reg, src, tgt, kw, r, f"{name} mode {mode}", score_mode=mode)


# ---- forced variants ---------------------------------------------------------------------------------------------------------
VARIANT_INPUTS = ["a:big:-30", "a:big:30", "a:big:-48", "a:big:62", "b:minlen0", "b:minlen-sub", "b:deep", "b:far62", "c:20:22", "c:22:24", "c:24:20", "e"]


@pytest.mark.parametrize("name", VARIANT_INPUTS)
def test_stage_a_variants(pkg, O, name):
    """Both interior-tile forms in both tile heights, and the bit-rows-only form, against the same restatement values."""
    src, tgt, kw, ref = _ref(pkg, O, name)
    p = pkg.make_params(max_triangles=T, **kw)
    r = pkg.Registrar(0)
    try:
        for one_phase in (0, 1):
            for rows in (16, 32):
                r.set_debug(compat_one_phase=one_phase, compat_rows=rows)
                S, bits, deg = r.compat(src, tgt, p)
                assert np.array_equal(bits, ref["bits"]) and np.array_equal(deg, ref["deg"]), (name, one_phase, rows)
                assert np.array_equal(u32(S), u32(ref["S"])), (name, one_phase, rows)
        r.set_debug()
        _, bits, deg = r.compat(src, tgt, pkg.make_params(max_triangles=T, flags=pkg.SC_FLAG_NO_DENSE_S, **kw), want_S=False)
        assert np.array_equal(bits, ref["bits"]) and np.array_equal(deg, ref["deg"]), (name, "no dense S")
        _check_register(pkg, r, src, tgt, kw, ref["reg"], name + " no dense S", flags=pkg.SC_FLAG_NO_DENSE_S)
    finally:
        r.close()


def _ran(r, what, want):
    """The kernel stage C2 ran in the last call: the forced one, or the library declined it (the Gram filter after a failed probe of
    the matrix pipe falls back to the linear filter or the plain kernel) — never silently a third thing."""
    info = r.debug_last()
    print(what, "c2_kernel", info["c2_kernel"], "gram_guard", info["gram_guard"], "undecided", info["filter_undecided"], "recounts", info["filter_recounts"])
    declined = want == 2 and info["gram_guard"] == 2 and info["c2_kernel"] in (0, 1)
    assert info["c2_kernel"] == want or declined, (what, info["c2_kernel"], want)


@pytest.mark.parametrize("name", VARIANT_INPUTS)
def test_score_variants(pkg, O, name):
    """Stage C2 by each forced kernel — plain, linear filter, Gram filter — by the f32-MFMA body, and chosen blind (without the
    coordinate maxima) on a call large enough for the filters: every count and the key against the restatement's."""
    src, tgt, kw, ref = _ref(pkg, O, name)
    if not len(ref["Rt"]):
        print(name, "no triangle: nothing to score")   # (c:22:24, c:24:20: every src or tgt point is the same point)
        return
    p = pkg.make_params(max_triangles=T, **kw)
    r = pkg.Registrar(0)
    try:
        for flt, want in ((1, 0), (2, 1), (3, 2)):
            r.set_debug(score_filter=flt)
            cnt, key = r.score(src, tgt, p, ref["Rt"])
            assert np.array_equal(cnt, ref["cnt"]) and key == ref["best_key"], (name, "score_filter", flt)
            _ran(r, f"{name} score_filter {flt}", want)
            _check_register(pkg, r, src, tgt, kw, ref["reg"], f"{name} score_filter {flt}")
        for split in (96, 256):
            r.set_debug(score_split=split)
            cnt, key = r.score(src, tgt, p, ref["Rt"])
            assert np.array_equal(cnt, ref["cnt"]) and key == ref["best_key"], (name, "score_split", split)
            _ran(r, f"{name} score_split {split}", 0)
        # 90 112 hypotheses x n >= 2^27 tests: the size from which the library takes a filter by itself
        reps = -(-90112 // len(ref["Rt"]))
        Rt = np.tile(ref["Rt"], (reps, 1))[:90112]; cnt0 = np.tile(ref["cnt"], reps)[:90112]
        pb = pkg.make_params(max_triangles=90112, **kw)
        r.set_debug()
        cnt, key = r.score(src, tgt, pb, Rt)
        assert np.array_equal(cnt, cnt0) and key == O.best_key(cnt0), (name, "large, by size and scale")
        print(name, "large call, by size and scale: c2_kernel", r.debug_last()["c2_kernel"])
        r.set_debug(filter_blind=1)
        cnt, key = r.score(src, tgt, pb, Rt)
        assert np.array_equal(cnt, cnt0) and key == O.best_key(cnt0), (name, "large, blind")
        _ran(r, f"{name} large call, blind", 1)          # not knowing the maxima, the host assumes the linear filter applies
    finally:
        r.close()


@pytest.mark.parametrize("k", [0, -40, 40, -60, 60])
def test_degenerate_triangles_at_every_scale(pkg, O, reg, k):
    """Duplicate vertices, an exactly collinear triangle, coincident target points: the Kabsch stage's bits, NaN rows included."""
    src, tgt, tri = degenerate_triangles(pkg)
    src, tgt = scaled(src, k), scaled(tgt, k)
    Rt0 = O.kabsch3(src, tgt, tri)
    Rt = reg.kabsch(src, tgt, pkg.make_params(max_triangles=T, **scaled_kw(k)), tri)
    bad = np.nonzero(~((np.isnan(Rt) & np.isnan(Rt0)) | (Rt.view(np.uint32) == Rt0.view(np.uint32))).all(1))[0]
    print("k", k, "NaN rows", np.nonzero(np.isnan(Rt0).any(1))[0].tolist(), "rows that differ", bad[:10].tolist())
    assert nan_equal_bits(Rt, Rt0)
    assert np.isnan(Rt0[50]).all() and np.isnan(Rt0[51]).all() and np.isfinite(Rt0).all(1).sum() == 4998


@pytest.mark.parametrize("name", [v.replace("a:big", "a:ragged") for v in VARIANT_INPUTS])
def test_refine_and_peel(pkg, O, name):
    """SC_FLAG_REFINE against O.refine, and the frame + two sc_peel rounds against the composition of tests/test_gpu_peel.py.  (Family a
    on the ragged scene: the big one's 3000 best triangles all lie in its translation block, whose 200 points the frame claims, and
    every later round is SC_ENOHYP.)"""
    src, tgt, kw, ref = _ref(pkg, O, name)
    r = pkg.Registrar(0)
    try:
        base = _check_register(pkg, r, src, tgt, kw, ref["reg"], name)
        got = r.register(src, tgt, flags=pkg.SC_FLAG_REFINE, max_triangles=T, **kw)
        assert got["status"] == base["status"] and np.array_equal(got["mask"], base["mask"]), name
        Rt12 = np.concatenate([base["R"].ravel(), base["t"]]).astype(np.float32)
        if base["status"] == 0:
            done, Rt0 = O.refine(src, tgt, base["mask"], Rt12)
            print(name, "refit done:", done)
            assert nan_equal_bits(np.concatenate([got["R"].ravel(), got["t"]]), Rt0 if done else Rt12), name
            kwp = dict(kw, max_triangles=T)
            with np.errstate(over="ignore", under="ignore"):
                exp, hyp = _expected(O, "range " + name, src, tgt, kwp, 3)
            _assert_rounds(_host_rounds(r, src, tgt, pkg.make_params(**kwp), 3), exp, hyp, name)
        else:
            assert nan_equal_bits(np.concatenate([got["R"].ravel(), got["t"]]), Rt12), name
    finally:
        r.close()


@pytest.mark.parametrize("name", ["a:big:30", "a:ragged:-48", "b:minlen0"])
def test_device_entries_warm_context(pkg, O, name):
    """One context taken through sc_register_device (the first call waits, repeats are enqueued host-free: the coordinate maxima
    arrive late there) and then sc_register_device_async + sc_wait: every call's outputs are the restatement's."""
    import torch
    dev = torch.device("cuda:0")
    src, tgt, kw, ref = _ref(pkg, O, name)
    n, r0 = len(src), ref["reg"]
    ds, dt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    p = pkg.make_params(max_triangles=T, **kw)
    want = np.concatenate([r0["R"].ravel(), r0["t"]])
    r = pkg.Registrar(0)
    try:
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        paths = []
        for call in range(5):
            d_Rt = torch.zeros(12, dtype=torch.float32, device=dev)
            d_mask = torch.full((n,), 7, dtype=torch.uint8, device=dev)
            if call < 3:
                rc, st = r.register_device(ds.data_ptr(), dt.data_ptr(), n, p, d_Rt.data_ptr(), d_mask.data_ptr())
            else:
                r.register_device_async(ds.data_ptr(), dt.data_ptr(), n, p, d_Rt.data_ptr(), d_mask.data_ptr())
                rc, st = r.wait()
            torch.cuda.synchronize()
            paths.append(r.debug_last()["fast_path"])
            assert rc == r0["rc"], (name, call)
            assert (st["edges"], st["tri_kept"], st["best_rank"], st["best_count"]) == (r0["edges"], r0["t_eff"], r0["best_rank"], r0["best_count"]), (name, call)
            assert np.array_equal(d_mask.cpu().numpy(), r0["mask"]) and nan_equal_bits(d_Rt.cpu().numpy(), want), (name, call)
        print(name, "fast_path per call:", paths)
        assert paths[0] == 0 and all(f in (1, 2) for f in paths[1:]), paths     # repeats of a shape are enqueued host-free
    finally:
        r.close()
