"""GPU: every host form of stage B through "grow, outgrow, come back" on one context.

Stage B's host side (csrc/sc_capi_tri.hip) decides a form per call — fused edge kernel or the separate ones, events or row walking,
estimated or certified bound, ordinals from the ordered strong list or from the scan, waited or host-free — and grows about twenty
arrays by two rules: "need now, room for the next host-free call" and "an array that was re-allocated lost what the speculative
launch wrote".  The other GPU files meet these in scattered places; this one runs each form through the same five calls on a fresh
context: small, large, small, small, small.

The small scene is just over the 4096 edges pruning needs.  The large one is beyond everything a young shape's room leaves after the
small one (2 x count + 4096, and the 64 KiB minimum allocation holds 16 384 edge entries): every edge-indexed and key-indexed array
is re-allocated in the second call and the speculative launches' output is void.  The third call comes back to arrays that are far
larger than it needs; the fourth and fifth repeat its shape, which is what a host-free enqueue waits for.

Every call is compared through the whole path with the CPU restatement, bit for bit.  What sc_debug_last says about the form that
ran — ordinals, prune_bound, fast_path, n_hostfree_grow — is pinned per form and call in EXPECTED: recorded data, not logic that
mirrors the library's conditions.
"""
import numpy as np
import pytest

from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

BASE = dict(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05, max_triangles=1000, rank_mode=0)
SCENES = {"small": 300, "large": 800}                      # synth.make_scene(n, 0.3, 1.0, 0.05, 7)
COUNTS = {"small": (4401, 42316), "large": (29584, 686413)}  # (edges, triangles) under BASE, from the CPU restatement
SEQUENCE = ("small", "large", "small", "small", "small")

# form -> (sc_set_debug knobs, sc_params overrides, SC_FLAG_* names)
FORMS = {
    "defaults": ({}, {}, ()),
    "no_events": (dict(no_events=1), {}, ()),
    "no_estimate": (dict(no_estimate=1), {}, ()),
    "no_edge_build": (dict(no_edge_build=1), {}, ()),
    "rows_unfused": (dict(rows_unfused=1), {}, ()),
    "scan_ordinals": (dict(scan_ordinals=1), {}, ()),
    "sample_mode_1": (dict(sample_mode=1), {}, ()),
    "sample_mode_2": (dict(sample_mode=2), {}, ()),
    "event_cap_256": (dict(event_cap=256), {}, ()),
    "compact_self_max_0": (dict(compact_self_max=0), {}, ()),
    "no_fast": (dict(no_fast=1), {}, ()),
    "exact_total": ({}, {}, ("SC_FLAG_EXACT_TOTAL",)),
    "no_prune": ({}, {}, ("SC_FLAG_NO_PRUNE",)),
    "rank_degree": ({}, dict(rank_mode=1), ()),
    "t_cmp_0.5": ({}, dict(t_cmp=0.5), ()),
}

# form -> per call of SEQUENCE: (ordinals, prune_bound, fast_path, n_hostfree_grow) of sc_debug_last
EXPECTED = {
    "defaults": [(0, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 0)],
    "no_events": [(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)],
    "no_estimate": [(0, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0)],
    "no_edge_build": [(0, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 0)],
    "rows_unfused": [(0, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 0)],
    "scan_ordinals": [(0, 1, 0, 0), (0, 1, 0, 0), (0, 1, 0, 0), (0, 1, 1, 0), (0, 1, 1, 0)],
    "sample_mode_1": [(0, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0)],
    "sample_mode_2": [(0, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0)],
    "event_cap_256": [(2, 2, 0, 0), (2, 0, 0, 0), (2, 0, 0, 0), (2, 0, 0, 0), (2, 0, 0, 0)],
    "compact_self_max_0": [(0, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 0)],
    "no_fast": [(0, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0)],
    "exact_total": [(0, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0)],
    "no_prune": [(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)],
    "rank_degree": [(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)],
    "t_cmp_0.5": [(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)],
}


def _kw(form):
    return dict(BASE, **FORMS[form][1])


def run_form(pkg, form):
    """The five calls of `form` on a fresh context: [(scene name, sc_register's result, sc_debug_last's)]."""
    knobs, _, flag_names = FORMS[form]
    flags = 0
    for f in flag_names:
        flags |= getattr(pkg, f)
    kw = _kw(form)
    out = []
    r = pkg.Registrar(0)
    try:
        if knobs:
            r.set_debug(**knobs)
        for name in SEQUENCE:
            sc = pkg.synth.make_scene(SCENES[name], 0.3, 1.0, 0.05, 7)
            got = r.register(sc.src, sc.tgt, flags=flags, **kw)
            out.append((name, got, r.debug_last()))
    finally:
        r.close()
    return out


def observed(info):
    return (info["ordinals"], info["prune_bound"], info["fast_path"], info["n_hostfree_grow"])


@pytest.fixture(scope="module")
def refs(pkg, O):
    """The CPU restatement's answer per (scene, distinct parameter set), computed once."""
    ref = {}
    for form in FORMS:
        kw = _kw(form)
        for name, n in SCENES.items():
            key = (name, tuple(sorted(kw.items())))
            if key not in ref:
                sc = pkg.synth.make_scene(n, 0.3, 1.0, 0.05, 7)
                ref[key] = O.register(sc.src, sc.tgt, threads=8, **kw)
    return ref


def test_the_scenes_have_the_counts_the_sequence_rests_on(refs):
    """small: just over the 4096 edges pruning needs; large: beyond a young shape's room after small, in edges and in keys."""
    base = tuple(sorted(BASE.items()))
    for name, (edges, tris) in COUNTS.items():
        assert (refs[(name, base)]["edges"], refs[(name, base)]["tri_total"]) == (edges, tris), name
    assert 4096 <= COUNTS["small"][0] and max(2 * COUNTS["small"][0] + 4096, 16384) < COUNTS["large"][0]
    assert 2 * COUNTS["small"][1] + 4096 < COUNTS["large"][1]


@pytest.mark.parametrize("form", list(FORMS))
def test_grow_outgrow_come_back(pkg, refs, form):
    kw = _kw(form)
    exact_total = "SC_FLAG_EXACT_TOTAL" in FORMS[form][2]
    seen = []
    for k, (name, got, info) in enumerate(run_form(pkg, form)):
        ref = refs[(name, tuple(sorted(kw.items())))]
        what = f"{form}, call {k} ({name})"
        assert got["status"] == ref["rc"] == 0, what
        st = got["stats"]
        assert (st["edges"], st["tri_kept"]) == (ref["edges"], ref["t_eff"]), what
        if exact_total:
            assert st["tri_total"] == ref["tri_total"], what
        assert (st["best_rank"], st["best_count"]) == (ref["best_rank"], ref["best_count"]), what
        assert np.array_equal(got["mask"], ref["mask"]), what
        assert nan_equal_bits(got["R"], ref["R"]) and nan_equal_bits(got["t"], ref["t"]), what
        seen.append(observed(info))
    print(f"{form}: {seen}")
    assert seen == EXPECTED[form], (form, seen, EXPECTED[form])
