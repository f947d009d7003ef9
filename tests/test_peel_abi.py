"""CPU suite: the surface of sc_peel (include/saccot.h) — the three exports, the Python mirror, and the synthetic
two-motion scenes the GPU tests of the rounds are built on.  No compute call is made: there is no GPU here."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_peel", "sc_peel_device", "sc_register_instances")


def test_peel_entries_are_exported_and_mirrored(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "saccot.h")).read()
    for name in NAMES:
        assert hasattr(L, name), f"libsaccot.so does not export {name}"
        assert name in pkg.api.EXPORTS and name + "(" in header
    assert L.sc_version() & 0xFFFF >= 9
    for method in ("peel", "peel_device", "register_instances"):
        assert callable(getattr(pkg.Registrar, method))


def test_registrar_still_fails_loudly_without_a_gpu(pkg):
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if have_gpu:  # (the suite also runs where there is one: the context then simply opens)
        pkg.Registrar(0).close()
        return
    with pytest.raises(pkg.SacCotError):
        pkg.Registrar(0)


def test_make_scene_motions_is_reproducible(pkg):
    S = pkg.synth
    cfg = S.CONFIGS["C1"]
    rhos = [0.6 * cfg.rho, 0.4 * cfg.rho]
    a = S.make_scene_motions(cfg.n, rhos, cfg.L, cfg.tau, cfg.seed)
    b = S.make_scene_motions(cfg.n, rhos, cfg.L, cfg.tau, cfg.seed)
    assert a.src.tobytes() == b.src.tobytes() and a.tgt.tobytes() == b.tgt.tobytes() and np.array_equal(a.label, b.label)
    assert a.src.dtype == np.float32 and a.tgt.shape == (cfg.n, 3) and a.label.dtype == np.int32 and len(a.motions) == 2
    assert ((a.label == 0).sum(), (a.label == 1).sum(), (a.label == -1).sum()) == (240, 160, 1600)
    # every true correspondence follows its own motion to within the noise (sigma = tau / 3, Irwin-Hall: |x| <= 6 sigma per axis)
    for k, (R, t) in enumerate(a.motions):
        own = a.label == k
        d = np.linalg.norm(a.src[own].astype(np.float64) @ R.T + t - a.tgt[own], axis=1)
        assert d.max() < 2 * np.sqrt(3) * cfg.tau + 1e-5
        other = a.label == 1 - k
        d = np.linalg.norm(a.src[other].astype(np.float64) @ R.T + t - a.tgt[other], axis=1)
        assert np.median(d) > 5 * cfg.tau
    # one motion: make_scene itself, bit for bit; the outliers and the source points never change
    one = S.make_scene_motions(cfg.n, [cfg.rho], cfg.L, cfg.tau, cfg.seed)
    ref = S.make_scene(cfg.n, cfg.rho, cfg.L, cfg.tau, cfg.seed)
    assert one.src.tobytes() == ref.src.tobytes() and one.tgt.tobytes() == ref.tgt.tobytes()
    assert np.array_equal(one.label == 0, ref.inlier) and a.src.tobytes() == ref.src.tobytes()
    out = a.label == -1
    assert a.tgt[out].tobytes() == ref.tgt[out].tobytes()
    c = S.make_scene_motions(cfg.n, rhos, cfg.L, cfg.tau, cfg.seed + 1)
    assert c.tgt.tobytes() != a.tgt.tobytes()


def test_make_scene_still_produces_the_golden_bits(pkg):
    g = np.load(os.path.join(ROOT, "tests", "golden", "c0.npz"))
    cfg, scene = pkg.synth.make_config_scene("C0")
    assert scene.src.tobytes() == np.ascontiguousarray(g["src"]).tobytes()
    assert scene.tgt.tobytes() == np.ascontiguousarray(g["tgt"]).tobytes()
