"""CPU suite: the CPU restatement (oracle/saccot_oracle.c) away from unit scale — against itself under exact power-of-two
scalings, and against the fp64 restatement (oracle/saccot_fp64.py) on scaled and on far-translated scenes.

tests/test_gpu_range.py pins the HIP path to the restatement on these magnitudes; that is only worth what the restatement is
worth out there, which is what this file checks.  It also owns the scenes and the windows below (test_gpu_range.py imports them).

Scale covariance.  Coordinates and the three length parameters (sigma, tau, min_len) times 2^k is an exact operation on fp32
data.  A stage is covariant at k when its outputs are those of k = 0, bit for bit (lengths: times 2^k exactly).  That holds
as long as every intermediate that can reach a result is a normal number; each window is derived from the stage's formulas for
the unit scenes below (extent 1, sigma = tau = min_len = 0.05, t_cmp = 0.9) and then confirmed by running the restatement at
EVERY k of the window (test_every_k_of_every_window) and on the GPU file's scenes at its k's (test_windows_hold_on_the_gpu_scenes).
"""
import math
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- the windows: inclusive ranges of k ----------------------------------------------------------------------------------
# Upper ends: the largest squared pair length / squared residual is < 2^3.2 at k = 0 (|q_i - q_j| < 3: asserted below), finite
# while 3.2 + 2k < 128.
# A, adjacency bits and degrees: the squared length of every pair that can pass min_len (>= 0.05^2 = 2^-8.6) stays normal:
#   -8.6 + 2k >= -126.
WIN_A_BITS = (-58, 62)
# A, weights: d * d stays normal wherever the weight is not exactly 1, i.e. |d^2 / (2 sigma^2)| > 2^-25 (below that sc_expf
#   returns 1 whatever the last bits of d * d are): d^2 > 2 * 0.05^2 * 2^-25 = 2^-32.6, so -32.6 + 2k >= -126.  (-1 / (2 sigma^2)
#   itself overflows only at k <= -61.)
WIN_A_S = (-46, 62)
# B: keys are sums of weights, which do not scale: stage B is covariant exactly where S is.
WIN_B = WIN_A_S
# C1 after the normalisation of kabsch3: only first powers of lengths are left (centroids, p - centroid, t = qc - R pc; R comes
#   from entries normalised to [1, 2) whatever k).  Sums reach 3 * 1.5 * 2^k (finite to k = 125); a product R_ij * pc_j of
#   the translation that can reach t's last bit is >= 2^-24 |t| >= 2^-24 * 2^-20 (|t| components > 2^-20 at k = 0: asserted
#   below), normal down to k = -82.
WIN_C1 = (-80, 120)
# C2 / C3: tau^2 = 2^-8.6 * 2^2k and the squared residuals next to it stay normal: as WIN_A_BITS.
WIN_C2 = (-58, 62)
# the whole path: the intersection
WIN_REGISTER = (max(WIN_A_S[0], WIN_C1[0], WIN_C2[0]), min(WIN_A_S[1], WIN_C1[1], WIN_C2[1]))

UNIT = dict(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05)


def in_window(k, win):
    return win[0] <= k <= win[1]


def pow2(k):
    """2^k as an fp32 value (exact for -149 <= k <= 127)."""
    return np.ldexp(np.float32(1), k)


def scaled(a, k):
    """a * 2^k in fp32: exact while the results are normal; overflows to inf / underflows like any fp32 product otherwise."""
    with np.errstate(over="ignore", under="ignore"):
        return (np.asarray(a, np.float32) * pow2(k)).astype(np.float32)


def scaled_kw(k, base=UNIT, **over):
    """The parameters with every length times 2^k (starting from the fp32 value of each, so that the scaling is exact)."""
    kw = dict(base)
    with np.errstate(over="ignore", under="ignore"):
        for name in ("sigma", "tau", "min_len"):
            kw[name] = float(np.float32(kw[name]) * pow2(k))
    kw.update(over)
    return kw


def scene_big(pkg):
    """N = 1500 (interior tiles of stage A in both heights), with exact duplicates and a pure-translation block as in
    tests/test_gpu_parity.py::test_compat_both_interior_forms_bit_exact: zero lengths, ties, d == 0."""
    sc = pkg.synth.make_scene(1500, 0.3, 1.0, 0.05, seed=77)
    src, tgt = sc.src.copy(), sc.tgt.copy()
    src[100:164] = src[36:100]; tgt[100:164] = tgt[36:100]
    tgt[200:400] = src[200:400] * np.float32(1.0) + np.float32(0.25)
    return src, tgt


def scene_ragged(pkg):
    """N = 1337: no multiple of any tile size."""
    sc = pkg.synth.make_scene(1337, 0.3, 1.0, 0.05, seed=5)
    return sc.src.copy(), sc.tgt.copy()


def scene_small(pkg):
    """N = 300: the scene every k of every window is run on."""
    sc = pkg.synth.make_scene(300, 0.4, 1.0, 0.05, 9)
    return sc.src.copy(), sc.tgt.copy()


def translated(src, tgt, es, et):
    """Both clouds moved far from the origin: + 2^es in src, + 2^et in tgt, rounded to fp32 (coordinates quantised to
    2^(es - 23) resp. 2^(et - 23))."""
    return (src + pow2(es)).astype(np.float32), (tgt + pow2(et)).astype(np.float32)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_nan(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint32) == b.view(np.uint32))))


def stages(O, src, tgt, kw, T, tri=None, threads=4):
    """Every stage of the restatement on one input -> dict.  `tri`: the triangles C1 runs on (default: this input's ranked list)."""
    with np.errstate(over="ignore", under="ignore"):        # (the binding squares tau in numpy: inf / 0 at the far k's, as the library's)
        return _stages(O, src, tgt, kw, T, tri, threads)


def _stages(O, src, tgt, kw, T, tri, threads):
    S, bits, deg = O.compat(src, tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"], threads=threads)
    tri_own, key, total = O.triangles(S, bits, deg, T, 0, threads=threads)
    tri = tri_own if tri is None else tri
    Rt = O.kabsch3(src, tgt, tri, threads=threads) if len(tri) else np.zeros((0, 12), np.float32)
    cnt = O.score(src, tgt, Rt, kw["tau"], threads=threads) if len(tri) else np.zeros(0, np.uint32)
    bk = O.best_key(cnt) if len(cnt) else 0
    mask = O.mask(src, tgt, Rt[0xFFFFFFFF - (bk & 0xFFFFFFFF)], kw["tau"]) if bk else np.zeros(len(src), np.uint8)
    reg = O.register(src, tgt, threads=threads, max_triangles=T, **kw)
    return dict(S=S, bits=bits, deg=deg, tri=tri_own, key=key, total=total, Rt=Rt, cnt=cnt, best_key=bk, mask=mask, reg=reg)


def assert_covariant(g, g0, k, what, a_bits=True, a_s=True, b=True, c1=True, c2=True, whole=True):
    """g: results at scale k, g0: at k = 0 (dicts of stages(), or the GPU's in the same shape).  Checks what the flags name."""
    f = pow2(k)
    if a_bits:
        assert np.array_equal(g["bits"], g0["bits"]) and np.array_equal(g["deg"], g0["deg"]), (what, k, "adjacency")
    if a_s:
        assert np.array_equal(u32(g["S"]), u32(g0["S"])), (what, k, "S")
    if b:
        assert g["total"] == g0["total"] and np.array_equal(g["key"], g0["key"]) and np.array_equal(g["tri"], g0["tri"]), (what, k, "ranked list")
    if c1:
        assert same_bits_nan(g["Rt"][:, :9], g0["Rt"][:, :9]), (what, k, "R")
        assert same_bits_nan(g["Rt"][:, 9:], g0["Rt"][:, 9:] * f), (what, k, "t")
    if c2:
        assert np.array_equal(g["cnt"], g0["cnt"]) and g["best_key"] == g0["best_key"] and np.array_equal(g["mask"], g0["mask"]), (what, k, "counts / mask")
    if whole:
        r, r0 = g["reg"], g0["reg"]
        assert (r["rc"], r["edges"], r["tri_total"], r["t_eff"], r["best_rank"], r["best_count"]) == \
               (r0["rc"], r0["edges"], r0["tri_total"], r0["t_eff"], r0["best_rank"], r0["best_count"]), (what, k, "register")
        assert np.array_equal(r["mask"], r0["mask"]) and same_bits_nan(r["R"], r0["R"]) and same_bits_nan(r["t"], r0["t"] * f), (what, k, "register R, t, mask")


# ---- precondition ---------------------------------------------------------------------------------------------------------
def test_this_process_keeps_fp32_subnormals(O):
    """A library loaded with flush-to-zero start-up code (-ffast-math's crtfastmath) would silently void every case below the
    normal range: numpy and the restatement must both still see subnormals."""
    assert np.float32(1e-40) * np.float32(0.5) != 0
    p = np.array([[0, 0, 0], [1e-20, 0, 0], [0, 1e-20, 0]], np.float32)     # squared lengths 1e-40, 2e-40: subnormal
    _, _, deg = O.compat(p, p, 1e-20, 0.9, 5e-21)
    assert deg.tolist() == [2, 2, 2]


# ---- the windows follow from the formulas ------------------------------------------------------------------------------------
def test_windows_follow_from_the_formulas(pkg, O):
    """Recomputes each window from the magnitudes the derivations at the top of the file name, on the scenes they are used on."""
    s2 = float(np.float32(UNIT["sigma"])) ** 2
    lo_len = math.ceil((-126 - math.log2(float(np.float32(UNIT["min_len"])) ** 2)) / 2)
    lo_s = math.ceil((-126 - math.log2(2 * s2 * 2.0 ** -25)) / 2)
    lo_tau = math.ceil((-126 - math.log2(float(np.float32(UNIT["tau"])) ** 2)) / 2)
    assert (WIN_A_BITS[0], WIN_A_S[0], WIN_C2[0]) == (lo_len, lo_s, lo_tau)
    for src, tgt in (scene_big(pkg), scene_ragged(pkg), scene_small(pkg)):
        ext = max(np.ptp(src.astype(np.float64), axis=0).max(), np.ptp(tgt.astype(np.float64), axis=0).max())
        assert ext < 3.0 and 3 * ext * ext < 2.0 ** 3.2 * 3                       # |x_i - x_j|^2 summed over three axes < 2^3.2 per axis bound
        hi = math.floor((128 - math.log2(3 * ext * ext) - 1e-9) / 2)
        assert hi >= WIN_A_BITS[1] == WIN_A_S[1] == WIN_C2[1]
        assert math.floor(127 - math.log2(3 * max(np.abs(src).max(), np.abs(tgt).max()))) >= WIN_C1[1]
    # C1's lower end: the translations of the small scene's hypotheses at k = 0
    src, tgt = scene_small(pkg)
    g0 = stages(O, src, tgt, UNIT, 2000)
    t = np.abs(g0["Rt"][np.isfinite(g0["Rt"]).all(1), 9:])
    assert t[t > 0].min() > 2.0 ** -20
    assert -126 + 24 + 20 <= WIN_C1[0]


# ---- covariance at every k --------------------------------------------------------------------------------------------------
def test_every_k_of_every_window(pkg, O):
    """N = 300, T = 2000: every stage at every k of its window equals k = 0.  C1 runs on the k = 0 ranked list and C2 on the k = 0
    hypotheses (t scaled), so that each stage's window is tested on its own and not through the narrower one before it."""
    src, tgt = scene_small(pkg)
    T = 2000
    g0 = stages(O, src, tgt, UNIT, T)
    assert g0["reg"]["rc"] == 0 and len(g0["tri"]) == T and g0["cnt"].max() > 50
    fin = np.isfinite(g0["Rt"]).all(1)
    assert fin.sum() > 0.95 * T
    wins = (WIN_A_BITS, WIN_A_S, WIN_C1, WIN_C2)
    for k in range(min(w[0] for w in wins), max(w[1] for w in wins) + 1):
        s, t = scaled(src, k), scaled(tgt, k)
        kw = scaled_kw(k)
        f = pow2(k)
        if in_window(k, WIN_A_BITS):
            S, bits, deg = O.compat(s, t, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"], threads=4)
            assert np.array_equal(bits, g0["bits"]) and np.array_equal(deg, g0["deg"]), k
            if in_window(k, WIN_A_S):
                assert np.array_equal(u32(S), u32(g0["S"])), k
                tri, key, total = O.triangles(S, bits, deg, T, 0, threads=4)
                assert total == g0["total"] and np.array_equal(tri, g0["tri"]) and np.array_equal(key, g0["key"]), k
        if in_window(k, WIN_C1):
            Rt = O.kabsch3(s, t, g0["tri"], threads=4)
            assert same_bits_nan(Rt[:, :9], g0["Rt"][:, :9]), k
            assert same_bits_nan(Rt[:, 9:], g0["Rt"][:, 9:] * f), k
        if in_window(k, WIN_C2):
            Rt = g0["Rt"].copy(); Rt[:, 9:] *= f
            cnt = O.score(s, t, Rt, kw["tau"], threads=4)
            assert np.array_equal(cnt, g0["cnt"]), k
            best = 0xFFFFFFFF - (g0["best_key"] & 0xFFFFFFFF)
            assert np.array_equal(O.mask(s, t, Rt[best], kw["tau"]), g0["mask"]), k
        if in_window(k, WIN_REGISTER):
            r, r0 = O.register(s, t, threads=4, max_triangles=T, **kw), g0["reg"]
            assert (r["rc"], r["edges"], r["tri_total"], r["best_rank"], r["best_count"]) == \
                   (r0["rc"], r0["edges"], r0["tri_total"], r0["best_rank"], r0["best_count"]), k
            assert np.array_equal(r["mask"], r0["mask"]) and same_bits_nan(r["R"], r0["R"]) and same_bits_nan(r["t"], r0["t"] * f), k
            if k % 8 == 0:                                                    # the fp64 refit has range to spare: a few k's
                Rt12 = np.concatenate([r0["R"].ravel(), r0["t"]])
                d0, f0 = O.refine(src, tgt, r0["mask"], Rt12)
                d1, f1 = O.refine(s, t, r["mask"], np.concatenate([r["R"].ravel(), r["t"]]))
                assert d0 and d1 and same_bits_nan(f1[:9], f0[:9]) and same_bits_nan(f1[9:], f0[9:] * f), k


GPU_KS = (-70, -64, -56, -50, -48, -47, -44, -40, -30, -20, 20, 30, 40, 50, 60, 62, 64, 66, 70)   # family a of tests/test_gpu_range.py


@pytest.mark.parametrize("which", ["big", "ragged"])
def test_windows_hold_on_the_gpu_scenes(pkg, O, which):
    """The scenes tests/test_gpu_range.py scales (N = 1500 with duplicates and a translation block, N = 1337), at those of its k's
    that lie in a window, and at the windows' ends: the metamorphic half of that file rests on this."""
    src, tgt = scene_big(pkg) if which == "big" else scene_ragged(pkg)
    T = 3000
    g0 = stages(O, src, tgt, UNIT, T, threads=8)
    assert g0["reg"]["rc"] == 0 and len(g0["tri"]) == T
    ks = sorted(set(k for k in GPU_KS if in_window(k, WIN_C1)) | {WIN_A_BITS[0], WIN_A_S[0], WIN_A_S[1]})
    for k in ks:
        g = stages(O, scaled(src, k), scaled(tgt, k), scaled_kw(k), T, tri=g0["tri"], threads=8)
        a_s = in_window(k, WIN_A_S)
        if not a_s:                                    # the ranked list of this k is not k = 0's: C2 on the k = 0 hypotheses
            Rt = g0["Rt"].copy(); Rt[:, 9:] *= pow2(k)
            with np.errstate(over="ignore", under="ignore"):
                g["cnt"] = O.score(scaled(src, k), scaled(tgt, k), Rt, scaled_kw(k)["tau"], threads=8)
                g["best_key"] = O.best_key(g["cnt"])
                g["mask"] = O.mask(scaled(src, k), scaled(tgt, k), Rt[0xFFFFFFFF - (g["best_key"] & 0xFFFFFFFF)], scaled_kw(k)["tau"])
        assert_covariant(g, g0, k, which, a_bits=in_window(k, WIN_A_BITS), a_s=a_s, b=a_s, c1=True,
                         c2=in_window(k, WIN_C2), whole=in_window(k, WIN_REGISTER))


def test_outside_the_windows_the_path_degrades_to_no_hypothesis(pkg, O):
    """What include/saccot.h promises outside: a pair whose squared length overflows is no edge, so the graph thins out (k = 66:
    only pairs shorter than 2^-2.4 are left) until nothing is left and the path reports SC_ENOHYP (k = 70: every pair that passes
    min_len overflows) — and the Kabsch stage no longer turns a registrable scene into NaN anywhere inside stage A's window (the
    bug this file's first version found: alpha = |H column|^2 is a fourth power of the triangle's size)."""
    src, tgt = scene_small(pkg)
    r0 = O.register(src, tgt, threads=4, max_triangles=2000, **UNIT)
    for k in (-44, -40, 40, 50, 62):
        r = O.register(scaled(src, k), scaled(tgt, k), threads=4, max_triangles=2000, **scaled_kw(k))
        assert r["rc"] == 0 and r["best_count"] == r0["best_count"] and np.isfinite(r["R"]).all(), k
    with np.errstate(over="ignore"):
        r = O.register(scaled(src, 66), scaled(tgt, 66), threads=4, max_triangles=2000, **scaled_kw(66))
        assert r["rc"] in (0, -5) and 0 < r["edges"] < r0["edges"] // 4 and np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all()
        r = O.register(scaled(src, 70), scaled(tgt, 70), threads=4, max_triangles=2000, **scaled_kw(70))
        assert r["rc"] == -5 and r["edges"] == 0 and np.array_equal(r["R"], np.eye(3)) and not r["mask"].any()


def degenerate_triangles(pkg):
    """The input of tests/test_gpu_parity.py::test_kabsch_bit_exact_random_and_degenerate: 5000 random triangles, 50 with a duplicate
    vertex (H of rank 1 up to rounding), one exactly collinear (rank 1 exactly), one with coincident target points (H = 0)."""
    sc = pkg.synth.make_scene(400, 0.3, 1.0, 0.05, 31)
    rng = np.random.default_rng(3)
    tri = np.sort(rng.integers(0, 400, (5000, 3)), axis=1).astype(np.uint32)
    tri[:50, 1] = tri[:50, 0]
    src, tgt = sc.src.copy(), sc.tgt.copy()
    src[:3] = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32); tri[50] = (0, 1, 2)
    tgt[3:6] = tgt[3]; tri[51] = (3, 4, 5)
    return src, tgt, tri


def test_degenerate_triangles_are_no_hypothesis_at_any_scale(pkg, O):
    """A triangle whose H has rank 1 exactly gives NaN (no hypothesis) whatever the unit of length — never a finite matrix that is no
    rotation (unnormalised, the vanishing column underflowed to 0 at unit scale and 0 / 0 said so; at 2^30 it did not) — and every
    finite result is a proper rotation."""
    src, tgt, tri = degenerate_triangles(pkg)
    Rt0 = O.kabsch3(src, tgt, tri)
    assert np.isnan(Rt0[50]).all() and np.isnan(Rt0[51]).all()
    good = np.isfinite(Rt0).all(1)
    assert good.sum() == 4998
    assert np.abs(np.linalg.det(Rt0[good, :9].reshape(-1, 3, 3).astype(np.float64)) - 1).max() < 1e-4
    for k in (-60, -40, -20, 20, 30, 40, 60):
        Rt = O.kabsch3(scaled(src, k), scaled(tgt, k), tri)
        assert same_bits_nan(Rt[:, :9], Rt0[:, :9]) and same_bits_nan(Rt[:, 9:], Rt0[:, 9:] * pow2(k)), k


# ---- against fp64 -----------------------------------------------------------------------------------------------------------
FP64_KS = (-40, -20, 20, 40, 60)


@pytest.mark.parametrize("k", FP64_KS)
def test_compat_against_fp64_scaled(pkg, O, k):
    """test_oracle.py::test_compat_against_fp64 with every length times 2^k; the fp64 side sees the scaled inputs."""
    from oracle import saccot_fp64 as F
    n, L = 300, 1.0
    sc = pkg.synth.make_scene(n, 0.3, L, 0.05, 5)
    src, tgt, kw = scaled(sc.src, k), scaled(sc.tgt, k), scaled_kw(k)
    S, bits, deg = O.compat(src, tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"])
    S64, A64, margin, deg64 = F.compat(src, tgt, kw["sigma"], kw["t_cmp"], kw["min_len"])
    A32 = S > 0
    unpacked = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)
    assert np.array_equal(unpacked, A32) and np.array_equal(deg, A32.sum(1))
    safe = margin > 1e-5 * L * 2.0 ** k
    assert np.array_equal(A32[safe], A64[safe])
    assert (~safe).sum() - n < 1e-3 * n * n
    both = A32 & A64
    assert both.sum() > 1000
    assert np.abs(S[both] - S64[both]).max() < 2e-6 + 2e-7 * L / 0.05            # weights do not scale
    assert np.array_equal(S, S.T)


@pytest.mark.parametrize("k", FP64_KS)
def test_kabsch_against_lapack_svd_scaled(pkg, O, k):
    """test_oracle.py::test_kabsch_against_lapack_svd at scale 2^k: R's tolerance is scale-free, t's is a length."""
    from oracle import saccot_fp64 as F
    sc = pkg.synth.make_scene(400, 1.0, 1.0, 0.02, 3)
    src, tgt = scaled(sc.src, k), scaled(sc.tgt, k)
    rng = np.random.default_rng(0)
    tri = np.sort(np.stack([rng.choice(400, 3, replace=False) for _ in range(600)]), axis=1).astype(np.uint32)
    Rt = O.kabsch3(src, tgt, tri)
    assert np.isfinite(Rt).all()
    worst_R = worst_t = 0.0
    checked = 0
    for h, (a, b, c) in enumerate(tri):
        R64, t64, s = F.kabsch(src[[a, b, c]], tgt[[a, b, c]])
        if s[1] < 0.05 * s[0]:
            continue
        checked += 1
        worst_R = max(worst_R, np.abs(Rt[h, :9].reshape(3, 3) - R64).max())
        worst_t = max(worst_t, np.abs(Rt[h, 9:] - t64).max())
    assert checked > 400
    assert worst_R < 2e-4 and worst_t < 2e-4 * 2.0 ** k
    R = Rt[:, :9].reshape(-1, 3, 3).astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5


@pytest.mark.parametrize("k", FP64_KS)
def test_score_against_fp64_residuals_scaled(pkg, O, k):
    """test_oracle.py::test_score_against_fp64_residuals at scale 2^k, on the hypotheses of the golden C0 triangles."""
    from oracle import saccot_fp64 as F
    cfg, sc = pkg.synth.make_config_scene("C0")
    g = np.load(os.path.join(GOLD, "c0.npz"))
    src, tgt = scaled(sc.src, k), scaled(sc.tgt, k)
    tau = float(np.float32(cfg.tau) * pow2(k))
    Rt = O.kabsch3(src, tgt, g["tri"])
    assert same_bits_nan(Rt[:, :9], g["Rt"][:, :9])                             # (the golden rotations, whatever the unit of length)
    cnt = O.score(src, tgt, Rt, tau)
    assert np.array_equal(cnt, g["cnt"])
    for h in range(len(Rt)):
        d2 = F.residual2(src, tgt, Rt[h, :9].reshape(3, 3), Rt[h, 9:])
        band = np.abs(d2 - tau * tau) <= 1e-4 * tau * tau
        lo = int((d2[~band] < tau * tau).sum())
        assert lo <= cnt[h] <= lo + int(band.sum())
    best = int(np.argmax(cnt))
    assert np.array_equal(O.mask(src, tgt, Rt[best], tau).sum(), cnt[best])


# Family c — far from the origin.  The unit scene collapses onto a handful of lattice points there (test_gpu_range.py runs exactly
# that, for parity); for a comparison with fp64 that leaves more than the guard band, the scene is larger: extent 2^16, sigma = tau =
# min_len = 2^8, moved by 2^20 / 2^22, so that the coordinates' ulp (2^-3 resp. 2^-1) is 1 / 512 of tau at most.
FAR = dict(L=65536.0, tau=256.0, es=20, et=22)


def _far_scene(pkg, n, rho, seed):
    sc = pkg.synth.make_scene(n, rho, FAR["L"], FAR["tau"], seed)
    src, tgt = translated(sc.src, sc.tgt, FAR["es"], FAR["et"])
    ulp = float(max(np.spacing(np.abs(src).max()), np.spacing(np.abs(tgt).max())))
    return sc, src, tgt, ulp


def test_compat_against_fp64_far_from_the_origin(pkg, O):
    """Same assertions and caps as test_compat_against_fp64; the guard band is one ulp of the coordinates instead of 1e-5 L."""
    from oracle import saccot_fp64 as F
    n, tau = 300, FAR["tau"]
    sc, src, tgt, ulp = _far_scene(pkg, n, 0.3, 5)
    assert ulp == 0.5
    S, bits, deg = O.compat(src, tgt, tau, 0.9, tau, tau)
    S64, A64, margin, deg64 = F.compat(src, tgt, tau, 0.9, tau)
    A32 = S > 0
    unpacked = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)
    assert np.array_equal(unpacked, A32) and np.array_equal(deg, A32.sum(1))
    safe = margin > ulp
    assert np.array_equal(A32[safe], A64[safe])
    assert (~safe).sum() - n < 1e-3 * n * n
    both = A32 & A64
    assert both.sum() > 1000
    assert np.abs(S[both] - S64[both]).max() < 2e-6 + 2e-7 * FAR["L"] / tau
    assert np.array_equal(S, S.T)


def test_kabsch_against_lapack_svd_far_from_the_origin(pkg, O):
    """R to the unit-scale tolerance (the centred triangle does not know where the origin is); t = qc - R pc inherits R's error
    times |pc|, so its tolerance is 2e-4 of the largest coordinate instead of 2e-4 of the unit extent."""
    from oracle import saccot_fp64 as F
    sc, src, tgt, ulp = _far_scene(pkg, 400, 1.0, 3)
    rng = np.random.default_rng(0)
    tri = np.sort(np.stack([rng.choice(400, 3, replace=False) for _ in range(600)]), axis=1).astype(np.uint32)
    Rt = O.kabsch3(src, tgt, tri)
    worst_R = worst_t = 0.0
    checked = 0
    for h, (a, b, c) in enumerate(tri):
        R64, t64, s = F.kabsch(src[[a, b, c]], tgt[[a, b, c]])
        if s[1] < 0.05 * s[0]:
            continue
        checked += 1
        worst_R = max(worst_R, np.abs(Rt[h, :9].reshape(3, 3) - R64).max())
        worst_t = max(worst_t, np.abs(Rt[h, 9:] - t64).max())
    assert checked > 400
    assert worst_R < 2e-4 and worst_t < 2e-4 * max(np.abs(src).max(), np.abs(tgt).max())


def test_score_against_fp64_residuals_far_from_the_origin(pkg, O):
    """The residual chain rounds four times per component at the size of the coordinates (<= ulp / 2 each, ulp of the LARGER cloud's
    coordinates; the products R p reach sqrt(3) times that): |d_fp32 - d_fp64| < 8 ulp.  Correspondences whose fp64 distance is within
    8 ulp of tau form the band; every other one must be counted as fp64 counts it."""
    from oracle import saccot_fp64 as F
    tau = FAR["tau"]
    sc, src, tgt, ulp = _far_scene(pkg, 500, 0.3, 1000)
    rng = np.random.default_rng(1)
    inl = np.nonzero(sc.inlier)[0]
    tri = np.sort(np.stack([rng.choice(inl if h % 2 else 500, 3, replace=False) for h in range(200)]), axis=1).astype(np.uint32)
    Rt = O.kabsch3(src, tgt, tri)
    cnt = O.score(src, tgt, Rt, tau)
    assert cnt.max() > 50
    for h in range(len(Rt)):
        if not np.isfinite(Rt[h]).all():
            assert cnt[h] == 0
            continue
        d = np.sqrt(F.residual2(src, tgt, Rt[h, :9].reshape(3, 3), Rt[h, 9:]))
        band = np.abs(d - tau) <= 8 * ulp
        lo = int((d[~band] < tau).sum())
        assert lo <= cnt[h] <= lo + int(band.sum())
        assert band.sum() <= 0.1 * len(d)
