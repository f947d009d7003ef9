"""GPU: the run-time guard of the Gram filter's silicon model, and a GPU-vs-GPU fuzz net around the filter.

The Gram filter (stage C2's default at the C2 / C4 sizes) is bit-exact only as long as one v_mfma_f32_32x32x16_f16 stays
within GX_ACC = 18.5 x 2^-24 of its largest term — a MEASURED property of gfx950's matrix pipe (sc_gram_guard.hip).  Every
context therefore probes its own pipe before the first call that would choose that filter (gram_guard_kernel); these
tests pin (a) what the probe reports on the box the suite runs on, (b) that a failing probe really takes the Gram filter
out of the path with identical results, and (c) Gram == fp32 kernel on clouds the synthetic BASELINE scenes never show
(ADVICE r03).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _params(tau, T):
    return dict(sigma=tau, t_cmp=0.9, tau=tau, min_len=tau, max_triangles=T, rank_mode=0)


def _rotations(rng, T):
    q = rng.normal(size=(T, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)


def _small_scene(rng, n=600):
    p = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    R = _rotations(rng, 1)[0].reshape(3, 3)
    q = (p.astype(np.float64) @ R.T + 0.3 + rng.normal(size=(n, 3)) * 0.02).astype(np.float32)
    return p, q, R


def test_matrix_pipe_probe_holds_on_this_silicon(pkg):
    """The probe itself: ~1e6 cancelling dot products against fp64.  The bound assumes 18.5 units of 2^-24 of the largest
    term; a context tolerates 9.25; r03's microbenchmark saw 3.75 over 15 000 products and the cut model of the pipe
    allows 17.  Here: the model holds, sub-normal fp16 operands are kept, and the worst case stays below a third of
    what the bound assumes — a pipe that rounds differently fails HERE, loudly, not in a parity scene that happens to
    land a test inside a mis-bounded sliver."""
    rng = np.random.default_rng(5)
    p, q, R = _small_scene(rng)
    T = 64
    Rt = np.concatenate([np.tile(R.ravel(), (T, 1)), np.full((T, 3), 0.3)], axis=1).astype(np.float32)
    r = pkg.Registrar(0)
    try:
        assert r.debug_last()["gram_guard"] == 0            # not probed before a call could choose the Gram filter
        r.set_debug(score_filter=3)
        r.score(p, q, pkg.make_params(**_params(0.1, T)), Rt)
        d = r.debug_last()
        assert d["c2_kernel"] == 2 and d["gram_guard"] == 1, d
        assert 0.0 < d["gram_guard_worst"] <= 18.5 / 3, d   # (0: nothing was compared)
        print("matrix-pipe probe: worst |hw - exact| / largest term =", d["gram_guard_worst"], "x 2^-24")
    finally:
        r.close()


def test_failing_probe_takes_the_gram_filter_out_of_the_path(pkg, O):
    """sc_debug.gram_guard_fail makes the probe report a violation: a call that would run the Gram filter — forced, or
    chosen by size at the C2 shape — runs the linear filter instead (c2_kernel == 1), with identical results."""
    rng = np.random.default_rng(6)
    p, q, R = _small_scene(rng, 900)
    T = 300
    Rt = np.concatenate([_rotations(rng, T) * 0 + R.ravel(), 0.3 + rng.normal(size=(T, 3)) * 0.05], axis=1).astype(np.float32)
    prm = pkg.make_params(**_params(0.1, T))
    r = pkg.Registrar(0)
    try:
        r.set_debug(score_filter=1)
        c_plain, k_plain = r.score(p, q, prm, Rt)
        r.set_debug(score_filter=3)
        c_g, k_g = r.score(p, q, prm, Rt)
        assert r.debug_last()["c2_kernel"] == 2
        r.set_debug(score_filter=3, gram_guard_fail=1)
        c_f, k_f = r.score(p, q, prm, Rt)
        d = r.debug_last()
        assert d["c2_kernel"] == 1 and d["gram_guard"] == 2, d
        assert np.array_equal(c_g, c_plain) and np.array_equal(c_f, c_plain) and k_g == k_plain == k_f
        assert c_plain.max() > 100
        # the whole path at the headline shape: chosen by size, then vetoed by the guard
        cfg, scene = pkg.synth.make_config_scene("C2")
        r.set_debug()
        a = r.register(scene.src, scene.tgt, **cfg.params())
        assert r.debug_last()["c2_kernel"] == 2
        r.set_debug(gram_guard_fail=1)
        b = r.register(scene.src, scene.tgt, **cfg.params())
        assert r.debug_last()["c2_kernel"] == 1
        assert np.array_equal(a["mask"], b["mask"]) and np.array_equal(a["R"].view(np.uint32), b["R"].view(np.uint32))
        assert a["stats"]["best_rank"] == b["stats"]["best_rank"] and a["stats"]["best_count"] == b["stats"]["best_count"]
    finally:
        r.close()


def _cloud(rng, kind, n):
    if kind == "clustered":      # a few tight clusters far apart
        k = int(rng.integers(2, 9))
        ctr = rng.uniform(-1, 1, (k, 3))
        p = ctr[rng.integers(0, k, n)] + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, -1)
    elif kind == "planar":       # z squeezed to almost nothing
        p = rng.uniform(-1, 1, (n, 3)); p[:, 2] *= 10.0 ** rng.uniform(-6, -2)
    elif kind == "collinear":    # along one (oblique) line, with a little scatter
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        p = rng.uniform(-1, 1, (n, 1)) * d + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-5, -2)
    elif kind == "duplicated":   # few distinct correspondences, many copies
        base = rng.uniform(-1, 1, (int(rng.integers(5, 60)), 3))
        p = base[rng.integers(0, len(base), n)]
    else:
        p = rng.uniform(-1, 1, (n, 3))
    return p


@pytest.mark.parametrize("block", range(4))
def test_gram_filter_equals_fp32_kernel_on_degenerate_clouds(pkg, block):
    """104 draws (4 x 26): clustered, planar, collinear, duplicated and uniform clouds, offset from the origin, at scales
    1e-4 .. 1e4, tau across the range in which the HOST's own rule picks the Gram filter, calls big enough (>= 2^27 tests)
    for that rule to apply; hypotheses far from the truth — random rotations, translations anywhere in the cloud — and, in
    every other draw, a quarter of them near it so that residuals land around tau.  Every count equals the fp32 kernel's;
    where the host chose the Gram filter and all hypotheses are far ones (rotations not further off than the clouds are
    wide), no (wave, split) may have been handed to the exact pass wholesale.  (With near-truth hypotheses at the small-tau end
    of the range a wave's queue of undecided tests can overflow — hundreds of residuals inside a shell 10 - 25 % of tau^2
    wide — and the filter then hands the wave over, as designed: no assertion on the recounts there.)"""
    rng = np.random.default_rng(9000 + block)
    reg = pkg.Registrar(0)
    plain = pkg.Registrar(0); plain.set_debug(score_filter=1)
    kinds = ["clustered", "planar", "collinear", "duplicated", "uniform"]
    chosen = near_seen = 0
    try:
        for it in range(26):
            kind = kinds[(it + block) % len(kinds)]
            n = int(rng.integers(1500, 9000))
            T = ((1 << 27) // n // 256 + 1 + int(rng.integers(0, 8))) * 256
            scale = float(10.0 ** rng.uniform(-4, 4))
            p = _cloud(rng, kind, n) + rng.uniform(-3, 3, 3)            # off-centre: the filter must centre it
            R = _rotations(rng, 1)[0].reshape(3, 3)
            t = rng.uniform(-2, 2, 3)
            half = 0.5 * float(np.max(p.max(0) - p.min(0)))
            tau = half * float(10.0 ** rng.uniform(np.log10(0.03), np.log10(0.45)))
            q = p @ R.T + t + rng.normal(size=(n, 3)) * tau * 0.4
            out = rng.random(n) < 0.4
            q[out] = q[~out].mean(0) + rng.uniform(-1, 1, (int(out.sum()), 3)) * half
            Rh = _rotations(rng, T)
            th = q.mean(0) - (Rh.reshape(T, 3, 3) @ p.mean(0)) + rng.uniform(-1, 1, (T, 3)) * half
            near = (rng.random(T) < 0.25) & (it % 2 == 1)                # odd draws: a quarter near the truth
            Rh[near] = R.ravel()
            th[near] = t + rng.normal(size=(int(near.sum()), 3)) * tau * 0.5
            Rt = np.concatenate([Rh, th], axis=1)
            src = (p * scale).astype(np.float32); tgt = (q * scale).astype(np.float32)
            Rt[:, 9:] *= scale
            Rt = Rt.astype(np.float32)
            prm = pkg.make_params(**_params(tau * scale, T))
            c_g, k_g = reg.score(src, tgt, prm, Rt)
            d = reg.debug_last()
            c_p, k_p = plain.score(src, tgt, prm, Rt)
            assert np.array_equal(c_g, c_p) and k_g == k_p, (block, it, kind, n, T, scale, tau / half, d)
            if d["c2_kernel"] == 2:
                chosen += 1
                if it % 2 == 0:
                    assert d["filter_recounts"] == 0, (block, it, kind, n, T, scale, tau / half, d)
                else:
                    near_seen += int(d["filter_undecided"] > 0)
        assert chosen >= 15 and near_seen >= 4, (chosen, near_seen)   # (the rule must really pick the Gram filter in most draws)
    finally:
        reg.close(); plain.close()
