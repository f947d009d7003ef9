"""GPU: the views of the row-indexed arrays (sc_kernels.hpp: RowStats, RowOffsets, ShardCut, ScanExtra) across frames that grow them.

A view holds plain pointers; a buffer that grows is freed and allocated again.  The host driver takes every view behind the last
ENSURE of what it names — a view kept across one would hand a launch the freed address.  This test makes every row-indexed array grow
under the launches that write it, on ONE context per form, and compares every frame with the CPU restatement, bit for bit.

A buffer's smallest allocation is 64 KiB, so:
  small -> mid   (ld 8000, W 125) grows bits, bits2 and wpre (4 MB); n = 8000 is the largest shape the fused row kernel takes (n <= 8192);
  mid -> large   (ld 16512, W 258) grows deg (66 000 B), degp, ebase, edge_off (132 008 B), wpre, scan_tmp and lb_state, and takes the
                 degrees through the tiled scans (n > 8192: the scan of deg+ writes ebase).  None of deg, degp, ebase, edge_off grows
                 before n passes 16 384: that is why the large frame is that large;
  large -> small comes back to arrays far larger than the frame needs.
mid and large run with SC_FLAG_NO_DENSE_S (S would be 256 MB and 1.09 GB; nothing after stage A reads it).

Forms (sc_set_debug): the fused edge kernel; no_edge_build — the fused row kernel up to 8192 rows, then row_stats plus the look-back
scan that writes ebase; no_edge_build + rows_unfused + scan_self_max = 0 — row_stats and the one-block scan below 8192, the
three-kernel scans above, and the per-edge count scans in three kernels throughout.
"""
import numpy as np
import pytest

from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

BASE = dict(t_cmp=0.9, rank_mode=0)
# name -> (synth.make_scene arguments, max_triangles, dense S?)
SCENES = {
    "small": ((300, 0.3, 1.0, 0.05, 7), 1000, True),
    "mid": ((8000, 0.08, 3.0, 0.1, 11), 6000, False),
    "large": ((16500, 0.05, 4.0, 0.1, 12), 6000, False),
}
COUNTS = {"small": (4401, 42316), "mid": (819623, 17267147), "large": (2317796, 37604746)}  # (edges, triangles), from the CPU restatement
SEQUENCE = ("small", "mid", "large", "small")
FORMS = {
    "edge_build": {},
    "no_edge_build": dict(no_edge_build=1),
    "rows_unfused_three_kernel_scans": dict(no_edge_build=1, rows_unfused=1, scan_self_max=0),
}


def _scene(pkg, name):
    args, T, _ = SCENES[name]
    tau = args[3]
    return pkg.synth.make_scene(*args), dict(BASE, sigma=tau, tau=tau, min_len=tau, max_triangles=T)


@pytest.fixture(scope="module")
def refs(pkg, O):
    """The CPU restatement's answer per scene, computed once."""
    ref = {}
    for name in SCENES:
        sc, kw = _scene(pkg, name)
        ref[name] = O.register(sc.src, sc.tgt, threads=8, **kw)
    return ref


def test_the_scenes_have_the_counts_the_sequence_rests_on(refs):
    """The three (edges, triangles) pairs, and that every frame fills its max_triangles hypotheses."""
    for name, (edges, tris) in COUNTS.items():
        assert (refs[name]["edges"], refs[name]["tri_total"]) == (edges, tris), name
        assert refs[name]["rc"] == 0 and refs[name]["t_eff"] == SCENES[name][1], name
    assert SCENES["mid"][0][0] <= 8192 < 16384 < SCENES["large"][0][0]


@pytest.mark.parametrize("form", list(FORMS))
def test_views_follow_the_row_arrays_when_frames_grow_them(pkg, refs, form):
    r = pkg.Registrar(0)
    try:
        if FORMS[form]:
            r.set_debug(**FORMS[form])
        for k, name in enumerate(SEQUENCE):
            sc, kw = _scene(pkg, name)
            got = r.register(sc.src, sc.tgt, flags=0 if SCENES[name][2] else pkg.SC_FLAG_NO_DENSE_S, **kw)
            ref, st = refs[name], got["stats"]
            what = f"{form}, frame {k} ({name})"
            print(what, "status", got["status"], "edges", st["edges"], ref["edges"], "tri_kept", st["tri_kept"], ref["t_eff"],
                  "rank", st["best_rank"], ref["best_rank"], "count", st["best_count"], ref["best_count"])
            assert got["status"] == ref["rc"] == 0, what
            assert st["tri_kept"] == ref["t_eff"] == SCENES[name][1], what
            assert st["edges"] == ref["edges"] == COUNTS[name][0], what
            assert (st["best_rank"], st["best_count"]) == (ref["best_rank"], ref["best_count"]), what
            assert np.array_equal(got["mask"], ref["mask"]), what
            assert nan_equal_bits(got["R"], ref["R"]) and nan_equal_bits(got["t"], ref["t"]), what
    finally:
        r.close()
