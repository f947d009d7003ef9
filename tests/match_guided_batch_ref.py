"""The semantics of sc_match_guided_batch / sc_match_guided_pairs (include/saccot.h), composed from the restatements that exist:
per problem match_guided_ref.Problem (the guided matcher in numpy float32) under the problem's own pose, laid into match_batch_ref's
slots and count pairs; the pairs form goes through pairs_ref's expansion.  A problem whose input holds a non-finite value is (0, 1),
a problem whose record carries a status other than SC_OK — when the call reads it — is (0, 0), and neither writes anything into its
slot.  The reference of tests/test_gpu_match_guided_batch.py and tests/test_gpu_match_guided_pairs.py; every comparison against it
is bit for bit.  Also the batch and the table those tests share, so that tests/test_match_guided_batch_abi.py can check on the CPU
that they are what they are used for, and the helpers that carry a batch to the device entries."""
import numpy as np

import assign_ref as AR
import batch_ref
import match_guided_ref as MG
import pairs_ref

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
STATUS = 1  # SC_GUIDE_POSE_STATUS
FILL_I, FILL_F = -7, -3.0  # what the tests fill the outputs with before a call: nothing is written outside [slot, slot + n)
MIXED = ((1, 1), (3, 5), (65, 63), (130, 129), (300, 333))
POSE64 = np.dtype([("Rt", np.float32, 12), ("status", np.int32), ("rest", np.uint32, 3)])  # sc_polish_batch_result's head
POSE80 = batch_ref.RESULT_DTYPE  # sc_batch_result
assert POSE64.itemsize == 64 and POSE80.itemsize == 80


# ---- the reference ----------------------------------------------------------------------------------------------------------------
class Batch:
    """a list of match_guided_ref.Scene (each with its pose): the distances, residuals and masks of (problem, gate) are computed once
    and shared by the modes"""

    def __init__(self, scenes):
        self.scenes = list(scenes)
        self._prob = {}

    def __len__(self):
        return len(self.scenes)

    def problem(self, b, gate, Rt=None):
        sc = self.scenes[b]
        key = (b, gate, None if Rt is None else np.asarray(Rt, np.float32).tobytes())
        if key not in self._prob:
            self._prob[key] = MG.Problem(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, sc.Rt if Rt is None else Rt, gate)
        return self._prob[key]

    def offsets(self):
        so = np.concatenate([[0], np.cumsum([len(s.fsrc) for s in self.scenes])]).astype(np.uint32)
        to = np.concatenate([[0], np.cumsum([len(s.ftgt) for s in self.scenes])]).astype(np.uint32)
        return so, to

    def packed(self, layout=0):
        """-> (src_pts, fsrc, tgt_pts, ftgt) of the packed entries, the points in `layout`"""
        sp, tp = np.concatenate([s.src_pts for s in self.scenes]), np.concatenate([s.tgt_pts for s in self.scenes])
        if layout:
            sp, tp = np.ascontiguousarray(sp.T), np.ascontiguousarray(tp.T)
        return sp, np.concatenate([s.fsrc for s in self.scenes]), tp, np.concatenate([s.ftgt for s in self.scenes])

    def poses(self, dtype=None, statuses=None):
        """the pose records: (B, 12) float32, or records of `dtype` (fields Rt, status) with the statuses given (default SC_OK) and
        every other byte a pattern the library must not care about"""
        rt = np.stack([np.asarray(s.Rt, np.float32) for s in self.scenes])
        if dtype is None:
            return rt
        rec = np.frombuffer(bytes([0xA5]) * (dtype.itemsize * len(rt)), dtype).copy()
        rec["Rt"] = rt
        rec["status"] = 0 if statuses is None else statuses
        return rec


def one(batch, b, gate, Rt=None, status=None, **mkw):
    """problem b under its pose (or Rt) -> (corr, d2, g2, n, flag); status: the record's, when the call reads it"""
    empty = (np.zeros((0, 2), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32), 0)
    if status is not None and status != SC_OK:
        return empty + (0,)
    sc = batch.scenes[b]
    pose = sc.Rt if Rt is None else Rt
    if not all(np.isfinite(np.asarray(a, np.float32)).all() for a in (sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, pose)):
        return empty + (1,)
    corr, d2, g2 = batch.problem(b, gate, Rt).match(**mkw)
    return corr, d2, g2, len(corr), 0


def lay(results, src_sizes, knn):
    """per-problem (corr, d2, g2, n, flag) -> (corr (slots, 2), d2, g2, count (B, 2)) as the entries leave arrays that were filled
    with FILL_I / FILL_F: problem b's entries from slot src_off[b] * knn, nothing else touched"""
    off = np.concatenate([[0], np.cumsum(src_sizes)]).astype(np.int64) * knn
    corr = np.full((off[-1], 2), FILL_I, np.int32); d2 = np.full(off[-1], FILL_F, np.float32); g2 = np.full(off[-1], FILL_F, np.float32)
    count = np.zeros((len(results), 2), np.uint32)
    for b, (c, d, g, n, flag) in enumerate(results):
        corr[off[b]: off[b] + n] = c; d2[off[b]: off[b] + n] = d; g2[off[b]: off[b] + n] = g
        count[b] = (n, flag)
    return corr, d2, g2, count


def match_batch(batch, gate, statuses=None, poses=None, **mkw):
    """the whole batch -> lay(...) of every problem alone; poses (B, 12): instead of the scenes' own"""
    knn = mkw.get("knn", 1)
    res = [one(batch, b, gate, None if poses is None else poses[b], None if statuses is None else int(statuses[b]), **mkw)
           for b in range(len(batch))]
    return lay(res, [len(s.fsrc) for s in batch.scenes], knn)


def same(got, exp, tag):
    """device or host outputs (corr, d2, g2 or None, count) against lay()'s, bit for bit"""
    print(tag, "count", np.asarray(got[3]).tolist())
    assert np.array_equal(got[3], exp[3]), tag
    assert np.array_equal(got[0], exp[0]), tag
    assert got[1].view(np.uint32).tobytes() == exp[1].view(np.uint32).tobytes(), tag
    if got[2] is not None:
        assert got[2].view(np.uint32).tobytes() == exp[2].view(np.uint32).tobytes(), tag


# ---- the batch the tests share ------------------------------------------------------------------------------------------------------
def skip_scene(D=33):
    """test_gpu_match_guided.py's cluster scene under the identity: source rows 0..127 in cluster A, 128..255 in B, 256..383 in C (no
    target near: two whole 64-row tiles admit nothing); target columns 0..63 near B, 64..127 near A, 128..191 in a cluster of
    their own (a column tile that every row tile skips)"""
    A, B, Cc, Dd = np.array([0.0, 0, 0]), np.array([50.0, 0, 0]), np.array([0, 80.0, 0]), np.array([0, 0, -90.0])
    cs = np.concatenate([np.tile(A, (128, 1)), np.tile(B, (128, 1)), np.tile(Cc, (128, 1))])
    ct = np.concatenate([np.tile(B, (64, 1)), np.tile(A, (64, 1)), np.tile(Dd, (64, 1))])
    return MG.clusters(302, cs, ct, D)


MIXED_N, SKIP_AT, HOSTILE_AT = len(MIXED), len(MIXED), len(MIXED) + 1
_SHARED = {}


def shared_batch(D):
    """the five mixed shapes (match_guided_ref.shared_scene: each with its own pose), the cluster problem, and (65, 63) under a
    hostile finite pose; built once per D, never modified"""
    if D not in _SHARED:
        scenes = [MG.shared_scene(ns, nt, D) for ns, nt in MIXED] + [skip_scene(D)]
        h = MG.shared_scene(65, 63, D)
        scenes.append(MG.Scene(h.src_pts, h.fsrc, h.tgt_pts, h.ftgt, AR.hostile()))
        _SHARED[D] = Batch(scenes)
    return _SHARED[D]


def mixed_batch(D):
    """the five mixed shapes alone (sharing the scenes, not the cache, of shared_batch)"""
    key = ("mixed", D)
    if key not in _SHARED:
        _SHARED[key] = Batch(shared_batch(D).scenes[:MIXED_N])
    return _SHARED[key]


def with_scene(batch, b, **changed):
    """a batch with problem b's arrays replaced (copies; the others shared): changed = {field: array}"""
    s = batch.scenes[b]
    new = MG.Scene(*[np.array(changed.get(k, getattr(s, k))) for k in ("src_pts", "fsrc", "tgt_pts", "ftgt", "Rt")])
    return Batch(batch.scenes[:b] + [new] + batch.scenes[b + 1:])


# ---- the table and the list of the pairs tests ----------------------------------------------------------------------------------------
PAIR_SIZES = (65, 63, 130, 129, 3)
# a pair twice (0 and 2), a self pair, two pairs sharing target set 3 (mutual: their column minima must not meet), both directions
PAIRS = np.array([(0, 1), (2, 3), (0, 1), (2, 2), (4, 3), (1, 0), (3, 4)], np.uint32)
_TABLE = None


def table():
    """-> pairs_ref's table dict (sets, pts, feat, set_off) of five sets in ONE frame — points in the unit cube, so under a pose near
    the identity and MG.GATE a row has no, one or a few admissible targets — plus poses (P, 12): a different small motion per pair"""
    global _TABLE
    if _TABLE is None:
        sets = []
        for n in PAIR_SIZES:
            rng = np.random.default_rng(8800 + n)
            sets.append((rng.random((n, 3)).astype(np.float32), rng.normal(size=(n, pairs_ref.DIM)).astype(np.float32)))
        set_off = np.concatenate([[0], np.cumsum([len(p) for p, _ in sets])]).astype(np.uint32)
        ident = AR.rt_of(np.eye(3), np.zeros(3))
        poses = AR.perturbed(ident, len(PAIRS), 41, angle=0.05, shift=0.02)
        _TABLE = dict(sets=sets, pts=np.concatenate([p for p, _ in sets]), feat=np.concatenate([f for _, f in sets]), set_off=set_off,
                      poses=np.ascontiguousarray(poses, np.float32))
    return _TABLE


def expand(tab, pairs, poses):
    """the list as a Batch of packed problems in list order, pair p under poses[p]"""
    return Batch([MG.Scene(ps, fs, pt, ft, poses[p]) for p, (ps, fs, pt, ft) in enumerate(pairs_ref.expand(tab, pairs))])


# ---- carrying a batch to the device entries (GPU tests only) --------------------------------------------------------------------------
def to_device(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]


def outputs(slots, nb):
    """device outputs filled with FILL_I / FILL_F (the count pairs with 7) -> (d_corr, d_d2, d_g2, d_count)"""
    import torch
    dev = torch.device("cuda:0")
    return (torch.full((max(slots, 1), 2), FILL_I, dtype=torch.int32, device=dev), torch.full((max(slots, 1),), FILL_F, dtype=torch.float32, device=dev),
            torch.full((max(slots, 1),), FILL_F, dtype=torch.float32, device=dev), torch.full((max(nb, 1), 2), 7, dtype=torch.int32, device=dev))


def fetch(out, slots, nb, want_g2=True):
    corr, d2, g2, cnt = (t.cpu().numpy() for t in out)
    if not want_g2:
        assert (g2 == np.float32(FILL_F)).all()  # a NULL d_g2: nothing is written
    return corr[:slots], d2[:slots], (g2[:slots] if want_g2 else None), cnt[:nb].view(np.uint32)


def run_device(pkg, r, batch, gate, poses=None, flags=0, layout=0, want_g2=True, **mkw):
    """sc_match_guided_batch_device on the current torch stream -> (corr, d2, g2 or None, count); poses: (B, 12) or records"""
    import torch
    m = pkg.api.make_match_params(batch.scenes[0].fsrc.shape[1], **mkw)
    g = pkg.make_guide_params(gate, layout, flags)
    so, to = batch.offsets()
    pose, stride = r._pose_records(batch.poses() if poses is None else poses, len(batch))
    d = to_device(batch.packed(layout))
    d_pose = torch.from_numpy(pose.view(np.uint8).reshape(-1)).to("cuda:0")
    slots = int(so[-1]) * m.knn
    out = outputs(slots, len(batch))
    torch.cuda.synchronize()
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        r.match_guided_batch_device(d[0].data_ptr(), d[1].data_ptr(), so, d[2].data_ptr(), d[3].data_ptr(), to, m, g, d_pose.data_ptr(), stride,
                                    out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr() if want_g2 else None, out[3].data_ptr())
        torch.cuda.synchronize()
    finally:
        r.set_stream(None)
    return fetch(out, slots, len(batch), want_g2)


def run_host(r, batch, gate, poses=None, flags=0, layout=0, want_g2=True, **mkw):
    """sc_match_guided_batch (host arrays) -> (corr, d2, g2 or None, count), the slots beyond a problem's count set to the fill
    values: the host form fetches whole arrays, and what lies behind a count is unspecified there"""
    so, to = batch.offsets()
    sp, fs, tp, ft = batch.packed(layout)
    corr, d2, g2, count = r.match_guided_batch(sp, fs, so, tp, ft, to, batch.poses() if poses is None else poses, gate=gate, layout=layout,
                                               flags=flags, want_g2=want_g2, **mkw)
    knn = mkw.get("knn", 1)
    keep = np.zeros(len(d2), bool)
    for b in range(len(batch)):
        keep[int(so[b]) * knn: int(so[b]) * knn + int(count[b, 0])] = True
    corr = np.where(keep[:, None], corr, FILL_I).astype(np.int32); d2 = np.where(keep, d2, np.float32(FILL_F)).astype(np.float32)
    if g2 is not None:
        g2 = np.where(keep, g2, np.float32(FILL_F)).astype(np.float32)
    return corr, d2, g2, count
