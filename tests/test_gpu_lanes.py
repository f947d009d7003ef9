"""GPU: a directly enqueued, host-free sc_register_device_async frame on a caller's stream runs on the context's LANE.

The lane is a private stream of the context beside the caller's: the frame is ordered after everything the caller enqueued on its
stream before the call (fork) and before everything it enqueues after sc_wait (join); in between it may overlap the frame of
another context of the same stream — that is what the headline stream of bench.py gains from.  Nothing a frame computes changes:
every output here is compared, bit for bit, with a waited sc_register_device call of the same scene (no_fast=1) on a context of
its own, and that path is what tests/test_gpu_parity.py pins to the CPU restatement.

Shapes: synth.make_stream_scenes("C1", 8) — n = 2000, T = 10 000, tens of thousands of edges: the smallest shipped shape whose
every scene meets the host-free form's conditions (E >= 4096, M >= T).  Every context is warmed with two calls of the shape, so
that the calls that follow are enqueued host-free.
"""
import numpy as np
import pytest

from conftest import nan_equal_bits

pytestmark = pytest.mark.gpu

SCENES = 8
STAT_KEYS = ("edges", "tri_total", "tri_kept", "tri_scored", "best_rank", "best_count")


class _Stream:
    """The scenes on the device and, per scene, what a waited call returns (computed once, never written again)."""

    def __init__(self, pkg):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.cfg, self.scenes = pkg.synth.make_stream_scenes("C1", SCENES)
        self.n = self.cfg.n
        self.p = pkg.make_params(**self.cfg.params())
        self.ds = [torch.from_numpy(s.src).to(self.dev) for s in self.scenes]
        self.dt = [torch.from_numpy(s.tgt).to(self.dev) for s in self.scenes]
        self.cfg0, scene0 = pkg.synth.make_config_scene("C0")
        self.p0 = pkg.make_params(**self.cfg0.params())
        self.ds0, self.dt0 = torch.from_numpy(scene0.src).to(self.dev), torch.from_numpy(scene0.tgt).to(self.dev)
        g = pkg.Registrar(0)
        try:
            g.set_debug(no_fast=1)   # every call of this context waits for stage B's counts
            g.set_stream(torch.cuda.current_stream().cuda_stream)
            self.ref = []
            for k in range(SCENES):
                self.ref.append(self.waited(g, self.ds[k], self.dt[k], self.n, self.p))
                assert g.debug_last()["fast_path"] == 0 and self.ref[-1]["rc"] == 0
                if k == 0:
                    self.polish0 = g.polish(candidates=8, max_iter=16)
            self.ref0 = self.waited(g, self.ds0, self.dt0, self.cfg0.n, self.p0)
        finally:
            g.close()

    def outs(self, n=None):
        return (self.torch.zeros(12, dtype=self.torch.float32, device=self.dev),
                self.torch.full((n or self.n,), 7, dtype=self.torch.uint8, device=self.dev))

    def waited(self, g, ds, dt, n, p):
        d_Rt, d_mask = self.outs(n)
        rc, st = g.register_device(ds.data_ptr(), dt.data_ptr(), n, p, d_Rt.data_ptr(), d_mask.data_ptr())
        self.torch.cuda.synchronize()
        return dict(rc=rc, st=st, Rt=d_Rt.cpu().numpy(), mask=d_mask.cpu().numpy())

    def context(self, pkg, caller_stream=True, warm_scene=0, **knobs):
        """A context on torch's current stream (or on its private one), warmed with two calls of the shape."""
        g = pkg.Registrar(0)
        if knobs:
            g.set_debug(**knobs)
        if caller_stream:
            g.set_stream(self.torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            got = self.waited(g, self.ds[warm_scene], self.dt[warm_scene], self.n, self.p)
            assert same(got, self.ref[warm_scene])
        assert g.debug_last()["fast_path"] == 1 and g.debug_last()["n_lane"] == 0   # (sc_register_device: host-free, never on a lane)
        return g


def same(a, b):
    return (a["rc"] == b["rc"] and all(a["st"][k] == b["st"][k] for k in STAT_KEYS)
            and np.array_equal(a["mask"], b["mask"]) and nan_equal_bits(a["Rt"], b["Rt"]))


@pytest.fixture(scope="module")
def S(pkg):
    return _Stream(pkg)


def _two_in_flight(S, pkg, n_frames, **knobs):
    """n_frames frames over the scenes, two contexts on torch's current stream, frame f + 1 enqueued before frame f is waited for."""
    torch = S.torch
    Rt = torch.zeros(n_frames, 12, dtype=torch.float32, device=S.dev)
    mask = torch.full((n_frames, S.n), 7, dtype=torch.uint8, device=S.dev)
    pair = [S.context(pkg, warm_scene=0, **knobs), S.context(pkg, warm_scene=1, **knobs)]
    try:
        def enqueue(f):
            k = f % SCENES
            pair[f & 1].register_device_async(S.ds[k].data_ptr(), S.dt[k].data_ptr(), S.n, S.p, Rt[f].data_ptr(), mask[f].data_ptr())
        stats = []
        enqueue(0)
        for f in range(1, n_frames + 1):
            if f < n_frames:
                enqueue(f)
            stats.append(pair[(f - 1) & 1].wait())
        torch.cuda.synchronize()
        info = [g.debug_last() for g in pair]
    finally:
        for g in pair:
            g.close()
    got_Rt, got_mask = Rt.cpu().numpy(), mask.cpu().numpy()
    frames = [dict(rc=rc, st=st, Rt=got_Rt[f], mask=got_mask[f]) for f, (rc, st) in enumerate(stats)]
    return frames, {k: sum(i[k] for i in info) for k in ("n_frames", "n_fast_ok", "n_fast_repeat", "n_lane")}


def test_frames_on_lanes_equal_the_waited_call_and_lanes_were_used(S, pkg):
    n_frames = 3 * SCENES
    frames, tot = _two_in_flight(S, pkg, n_frames)
    print("lanes on:", tot)
    for f, fr in enumerate(frames):
        assert same(fr, S.ref[f % SCENES]), f"frame {f} (scene {f % SCENES}) differs from the waited call"
    assert tot["n_frames"] == n_frames + 4, tot      # (two warming calls per context)
    assert tot["n_lane"] >= 16, tot
    assert tot["n_fast_repeat"] <= SCENES // 2, tot   # (tests/test_gpu_stream_distinct.py: FRAMES // 2 of the first pass)
    # the same loop with the lanes switched off: no frame on a lane, the same outputs bit for bit
    frames_off, tot_off = _two_in_flight(S, pkg, n_frames, no_lane=1)
    print("lanes off:", tot_off)
    assert tot_off["n_lane"] == 0, tot_off
    assert tot_off["n_fast_repeat"] <= SCENES // 2, tot_off
    for f, (a, b) in enumerate(zip(frames, frames_off)):
        assert a["rc"] == b["rc"] and all(a["st"][k] == b["st"][k] for k in STAT_KEYS), f
        assert a["mask"].tobytes() == b["mask"].tobytes() and a["Rt"].tobytes() == b["Rt"].tobytes(), f


def test_a_lane_frame_is_ordered_after_the_callers_stream_at_the_call(S, pkg):
    """The inputs are produced ON the caller's stream, behind a few milliseconds of unrelated work, and nothing is synchronised
    before the call: a lane that did not wait for the fork would read scene A (a wrong answer, never a fault)."""
    torch = S.torch
    A, B = 0, 5
    d_src, d_tgt = S.ds[A].clone(), S.dt[A].clone()
    d_Rt, d_mask = S.outs()
    a = torch.randn(4096, 4096, device=S.dev)
    b = torch.empty_like(a)
    torch.matmul(a, a, out=b)                       # (the BLAS library's one-time set-up is not part of the window)
    g = S.context(pkg, warm_scene=A)
    try:
        torch.cuda.synchronize()
        for _ in range(6):
            torch.matmul(a, a, out=b)
        d_src.copy_(S.ds[B]); d_tgt.copy_(S.dt[B])
        g.register_device_async(d_src.data_ptr(), d_tgt.data_ptr(), S.n, S.p, d_Rt.data_ptr(), d_mask.data_ptr())
        rc, st = g.wait()
        info = g.debug_last()
        torch.cuda.synchronize()
        got = dict(rc=rc, st=st, Rt=d_Rt.cpu().numpy(), mask=d_mask.cpu().numpy())
    finally:
        g.close()
    assert info["lane"] == 1 and info["n_lane"] == 1, info
    assert not same(S.ref[A], S.ref[B])             # (the two scenes are told apart by what is compared)
    assert same(got, S.ref[B]), "the frame did not see the inputs the caller's stream produced before the call"


def test_a_lane_frame_is_ordered_before_the_callers_stream_at_wait_and_across_reuse_of_its_outputs(S, pkg):
    """One context, one pair of output buffers: the caller's copies of frame 1's outputs — enqueued after its sc_wait, not
    synchronised — hold frame 1's, although frame 2 is enqueued into the same buffers at once (its fork follows the copies)."""
    torch = S.torch
    A, B = 2, 6
    d_Rt, d_mask = S.outs()
    g = S.context(pkg, warm_scene=A)
    try:
        g.register_device_async(S.ds[A].data_ptr(), S.dt[A].data_ptr(), S.n, S.p, d_Rt.data_ptr(), d_mask.data_ptr())
        rc1, st1 = g.wait()
        keep_mask, keep_Rt = d_mask.clone(), d_Rt.clone()
        g.register_device_async(S.ds[B].data_ptr(), S.dt[B].data_ptr(), S.n, S.p, d_Rt.data_ptr(), d_mask.data_ptr())
        rc2, st2 = g.wait()
        torch.cuda.synchronize()
        info = g.debug_last()
    finally:
        g.close()
    assert info["n_lane"] == 2, info
    first = dict(rc=rc1, st=st1, Rt=keep_Rt.cpu().numpy(), mask=keep_mask.cpu().numpy())
    second = dict(rc=rc2, st=st2, Rt=d_Rt.cpu().numpy(), mask=d_mask.cpu().numpy())
    assert not same(S.ref[A], S.ref[B])
    assert same(first, S.ref[A]), "the copies taken after sc_wait do not hold frame 1's outputs"
    assert same(second, S.ref[B])


def test_which_calls_take_a_lane(S, pkg):
    torch = S.torch
    d_Rt, d_mask = S.outs()

    def async_frame(g, k, p=None):
        g.register_device_async(S.ds[k].data_ptr(), S.dt[k].data_ptr(), S.n, p or S.p, d_Rt.data_ptr(), d_mask.data_ptr())
        rc, st = g.wait()
        torch.cuda.synchronize()
        return dict(rc=rc, st=st, Rt=d_Rt.cpu().numpy(), mask=d_mask.cpu().numpy()), g.debug_last()

    g = S.context(pkg, warm_scene=3)
    try:
        # sc_register_device on a caller's stream: async + wait in one call, host-free, no lane
        got = S.waited(g, S.ds[3], S.dt[3], S.n, S.p)
        info = g.debug_last()
        assert (info["fast_path"], info["lane"], info["n_lane"]) == (1, 0, 0) and same(got, S.ref[3]), info
        got, info = async_frame(g, 3)
        assert (info["fast_path"], info["lane"], info["n_lane"]) == (1, 1, 1) and same(got, S.ref[3]), info
        # the first async call of a new shape waits and takes none; the next one does
        p2 = pkg.make_params(**(S.cfg.params() | {"max_triangles": 8000}))
        first, i1 = async_frame(g, 3, p2)
        assert (i1["fast_path"], i1["lane"], i1["n_lane"]) == (0, 0, 1), i1
        second, i2 = async_frame(g, 3, p2)
        assert (i2["fast_path"], i2["lane"], i2["n_lane"]) == (1, 1, 2) and same(second, first), i2
    finally:
        g.close()
    # a context on its private stream is on a lane of its own already: nothing changes for it
    g = S.context(pkg, caller_stream=False, warm_scene=4)
    try:
        got, info = async_frame(g, 4)
        assert (info["fast_path"], info["lane"], info["n_lane"]) == (1, 0, 0) and same(got, S.ref[4]), info
    finally:
        g.close()


def test_what_follows_a_lane_frame(S, pkg):
    torch = S.torch
    d_Rt, d_mask = S.outs()

    def async_frame(g, k):
        g.register_device_async(S.ds[k].data_ptr(), S.dt[k].data_ptr(), S.n, S.p, d_Rt.data_ptr(), d_mask.data_ptr())
        rc, st = g.wait()
        info = g.debug_last()
        torch.cuda.synchronize()
        return dict(rc=rc, st=st, Rt=d_Rt.cpu().numpy(), mask=d_mask.cpu().numpy()), info

    g = S.context(pkg)
    try:
        # sc_polish on a lane frame returns what it returns on a waited frame of the scene (compared as tests/test_gpu_polish.py
        # compares two polishes of one frame: _same_polish)
        g.register_device_async(S.ds[0].data_ptr(), S.dt[0].data_ptr(), S.n, S.p, d_Rt.data_ptr(), d_mask.data_ptr())
        rc, _ = g.wait()
        assert rc == 0
        pol, exp = g.polish(candidates=8, max_iter=16), S.polish0
        assert g.debug_last()["n_lane"] == 1
        assert pol["status"] == exp["status"] and pol["n_cand"] == exp["n_cand"]
        assert pol["cand"].tobytes() == exp["cand"].tobytes()
        assert np.concatenate([pol["R"].ravel(), pol["t"]]).tobytes() == np.concatenate([exp["R"].ravel(), exp["t"]]).tobytes()
        assert np.array_equal(pol["mask"], exp["mask"])
        assert all(pol["stats"][f] == exp["stats"][f] for f in ("n",) + STAT_KEYS)
        # a waited call of another shape between two lane frames, and the lane frame after it
        got, info = async_frame(g, 1)
        assert info["lane"] == 1 and same(got, S.ref[1]), info
        got0 = S.waited(g, S.ds0, S.dt0, S.cfg0.n, S.p0)
        assert g.debug_last()["fast_path"] == 0 and same(got0, S.ref0)
        got, info = async_frame(g, 2)                # (the shape changed: this one waits)
        assert (info["fast_path"], info["lane"]) == (0, 0) and same(got, S.ref[2]), info
        got, info = async_frame(g, 2)
        assert (info["fast_path"], info["lane"]) == (1, 1) and same(got, S.ref[2]), info
        # sc_set_stream while a lane frame is outstanding is refused like every other entry; the frame is none the worse for it
        g.register_device_async(S.ds[6].data_ptr(), S.dt[6].data_ptr(), S.n, S.p, d_Rt.data_ptr(), d_mask.data_ptr())
        with pytest.raises(pkg.SacCotError) as ei:
            g.set_stream(None)
        assert ei.value.status == pkg.SC_EINVAL
        rc, st = g.wait()
        info = g.debug_last()
        torch.cuda.synchronize()
        assert info["lane"] == 1 and same(dict(rc=rc, st=st, Rt=d_Rt.cpu().numpy(), mask=d_mask.cpu().numpy()), S.ref[6]), info
        # sc_destroy with a lane frame outstanding drains the lane and returns
        g.register_device_async(S.ds[5].data_ptr(), S.dt[5].data_ptr(), S.n, S.p, d_Rt.data_ptr(), d_mask.data_ptr())
    finally:
        g.close()
    torch.cuda.synchronize()
    assert same(dict(rc=0, st=S.ref[5]["st"], Rt=d_Rt.cpu().numpy(), mask=d_mask.cpu().numpy()), S.ref[5])   # (it ran to its end)
