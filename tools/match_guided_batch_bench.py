#!/usr/bin/env python3
"""What re-matching a batch under a pose per problem costs, batched (include/saccot.h, sc_match_guided_batch) and streamed, inputs
resident in HBM.

  python tools/match_guided_batch_bench.py [--batches 16,256,2048] [--n 256] [--dim 33] [--gate 0.05] [--repeats 10] [--warmup 2]
                                           [--parent-lib PATH] [--out profiles/match_guided_batch.txt]

Per B: B problems of n x n keypoints with `dim`-component descriptors (32 distinct seeded scenes, repeated): source keypoints fill
the unit cube, 30 % of the target keypoints are posed, slightly noisy copies of source keypoints with noisy descriptor copies, the
rest fill the posed cube; every problem's pose record is its true pose a little off.  The gate is `gate` x the extent of the cloud.
Two variants (knn 1, plain and SC_MATCH_MUTUAL) and two keypoint orders: random, and Morton order (each side sorted by the Morton
code of its own coordinates in its own bounding box — what a detector that walks an octree or an image pyramid delivers).  Routes,
timed in the same process in interleaved rounds (every route once per round, the order reversed every other round, so that no
route always runs behind the same neighbour) by a HIP event pair on the context's stream, `repeats` rounds after `warmup`,
min / median / max in microseconds PER PROBLEM:
  (a)       one sc_match_guided_batch_device call;
  (a_open)  the same with a gate that admits everything: the work of (c) plus the gate;
  (b)       sc_match_guided_device per problem, streamed on one context: what a caller had before the batch entry;
  (c)       one sc_match_batch_device call on the same descriptors, on a context of its own: the unguided kernel of this library,
  (c_parent) ... and of a library built from the parent commit (--parent-lib; omitted: not measured).
same: the slots of (a) equal those of (b) byte for byte within every problem's count.  tiles_skipped: the share of 64 x 64 tiles
in which no cell is admissible (fp64 on the host over the distinct scenes: a statistic, not the kernel's decision).  Prints one
JSON line per (B, order, variant), then a table; --out receives both.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

DISTINCT = 32
GATE_OPEN = 1e18


def morton(pts):
    """the order of the points by the Morton code (10 bits an axis) of their coordinates in their own bounding box"""
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    q = np.minimum(((pts - lo) / np.maximum(hi - lo, 1e-30) * 1024).astype(np.uint64), 1023)
    code = np.zeros(len(pts), np.uint64)
    for bit in range(10):
        for ax in range(3):
            code |= ((q[:, ax] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + ax)
    return np.argsort(code, kind="stable")


def scene(n, dim, seed, order, rho=0.3):
    """-> (src_pts, fsrc, tgt_pts, ftgt, Rt): the pose record is the true pose off by about 0.01 rad and 0.005 of the extent"""
    rng = np.random.default_rng(seed)
    src = rng.random((n, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    R = q * np.sign(np.linalg.det(q))
    t = rng.uniform(-1, 1, size=3)
    tgt = rng.random((n, 3)) @ R.T + t
    fsrc = rng.normal(size=(n, dim))
    ftgt = rng.normal(size=(n, dim))
    k = int(round(rho * n))
    rows = rng.permutation(n)[:k]
    tgt[:k] = src[rows] @ R.T + t + 0.002 * rng.normal(size=(k, 3))
    ftgt[:k] = fsrc[rows] + 0.05 * rng.normal(size=(k, dim))
    perm = rng.permutation(n)
    tgt, ftgt = tgt[perm], ftgt[perm]
    if order == "morton":
        a, b = morton(src), morton(tgt)
        src, fsrc, tgt, ftgt = src[a], fsrc[a], tgt[b], ftgt[b]
    w = rng.normal(size=3) * 0.01
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    dR = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th**2 * (K @ K)
    Rt = np.concatenate([(dR @ R).ravel(), dR @ t + 0.005 * rng.normal(size=3)])
    return [np.ascontiguousarray(x, np.float32) for x in (src, fsrc, tgt, ftgt, Rt)]


def tiles_skipped(scenes, gate):
    skipped = total = 0
    for src, _, tgt, _, Rt in scenes:
        R, t = Rt[:9].reshape(3, 3).astype(np.float64), Rt[9:].astype(np.float64)
        e = (src.astype(np.float64) @ R.T + t)[:, None, :] - tgt.astype(np.float64)[None, :, :]
        adm = (e * e).sum(axis=2) < gate * gate
        ns, nt = adm.shape
        for i in range(0, ns, 64):
            for j in range(0, nt, 64):
                total += 1
                skipped += not adm[i: i + 64, j: j + 64].any()
    return skipped / total


class ParentLib:
    """sc_match_batch_device of another build of the library (the parent commit's), on a context and a stream of its own handle"""

    def __init__(self, path, stream_ptr):
        self.L = C.CDLL(path)
        vp, u32p = C.c_void_p, C.POINTER(C.c_uint32)
        self.L.sc_create.argtypes = [C.c_int, C.POINTER(vp)]
        self.L.sc_destroy.argtypes = [vp]; self.L.sc_destroy.restype = None
        self.L.sc_set_stream.argtypes = [vp, vp]
        self.L.sc_match_batch_device.argtypes = [vp, vp, u32p, vp, u32p, C.c_uint32, vp, vp, vp, vp]
        self.h = vp()
        if self.L.sc_create(0, C.byref(self.h)) != 0 or self.L.sc_set_stream(self.h, stream_ptr) != 0:
            raise RuntimeError("the parent library refused sc_create / sc_set_stream")

    def match_batch_device(self, d_fsrc, off, d_ftgt, mp, d_corr, d_d2, d_count):
        o = off.ctypes.data_as(C.POINTER(C.c_uint32))
        if self.L.sc_match_batch_device(self.h, d_fsrc, o, d_ftgt, o, len(off) - 1, C.byref(mp), d_corr, d_d2, d_count) != 0:
            raise RuntimeError("the parent library refused sc_match_batch_device")

    def close(self):
        self.L.sc_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,256,2048")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--dim", type=int, default=33)
    ap.add_argument("--gate", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_guided_batch.txt"))
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    n, dim = a.n, a.dim
    reg = pkg.Registrar(0)
    stream = torch.cuda.Stream(device=dev)
    reg.set_stream(stream.cuda_stream)
    reg_c = pkg.Registrar(0)  # (c) on a context of its own, as the parent library's: the two are compared like for like
    reg_c.set_stream(stream.cuda_stream)
    parent = ParentLib(a.parent_lib, stream.cuda_stream) if a.parent_lib else None
    rows, lines = [], []
    try:
        for order in ("random", "morton"):
            scenes = [scene(n, dim, 9100 + k, order) for k in range(DISTINCT)]
            skipped = tiles_skipped(scenes, a.gate)
            for B in (int(x) for x in a.batches.split(",")):
                pack = [np.concatenate([scenes[b % DISTINCT][k] for b in range(B)]) for k in range(5)]
                d_src, d_fsrc, d_tgt, d_ftgt, d_pose = (torch.from_numpy(x).to(dev) for x in pack)
                off = (np.arange(B + 1, dtype=np.uint64) * n).astype(np.uint32)
                for variant, mkw in (("knn1", dict(knn=1)), ("knn1_mutual", dict(knn=1, mutual=True))):
                    mp = pkg.api.make_match_params(dim, **mkw)
                    g, g_open = pkg.make_guide_params(a.gate), pkg.make_guide_params(GATE_OPEN)
                    out = {k: (torch.zeros((B * n, 2), dtype=torch.int32, device=dev), torch.zeros(B * n, dtype=torch.float32, device=dev),
                               torch.zeros(B * n, dtype=torch.float32, device=dev), torch.zeros((B, 2), dtype=torch.int32, device=dev))
                           for k in ("a", "a_open", "b", "c", "c_parent")}
                    torch.cuda.synchronize()

                    def guided(o, gp):
                        reg.match_guided_batch_device(d_src.data_ptr(), d_fsrc.data_ptr(), off, d_tgt.data_ptr(), d_ftgt.data_ptr(), off, mp, gp,
                                                      d_pose.data_ptr(), 48, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr())

                    def streamed(o):
                        for b in range(B):
                            reg.match_guided_device(d_src.data_ptr() + b * n * 12, d_fsrc.data_ptr() + b * n * dim * 4, n, d_tgt.data_ptr() + b * n * 12,
                                                    d_ftgt.data_ptr() + b * n * dim * 4, n, mp, g, d_pose.data_ptr() + b * 48,
                                                    o[0].data_ptr() + b * n * 8, o[1].data_ptr() + b * n * 4, o[2].data_ptr() + b * n * 4,
                                                    o[3].data_ptr() + b * 8)

                    routes = {"a": lambda: guided(out["a"], g), "a_open": lambda: guided(out["a_open"], g_open), "b": lambda: streamed(out["b"]),
                              "c": lambda: reg_c.match_batch_device(d_fsrc.data_ptr(), off, d_ftgt.data_ptr(), off, mp, out["c"][0].data_ptr(),
                                                                  out["c"][1].data_ptr(), out["c"][3].data_ptr())}
                    if parent:
                        routes["c_parent"] = lambda: parent.match_batch_device(d_fsrc.data_ptr(), off, d_ftgt.data_ptr(), mp, out["c_parent"][0].data_ptr(),
                                                                               out["c_parent"][1].data_ptr(), out["c_parent"][3].data_ptr())
                    t = {k: [] for k in routes}
                    for it in range(a.warmup + a.repeats):  # interleaved rounds: every route once per round, the order reversed every other round
                        for k, fn in (list(routes.items()) if it % 2 == 0 else reversed(list(routes.items()))):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(stream)
                            fn()
                            e1.record(stream)
                            e1.synchronize()
                            if it >= a.warmup:
                                t[k].append(e0.elapsed_time(e1) * 1e3)
                    torch.cuda.synchronize()
                    ca, cb = out["a"][3].cpu().numpy(), out["b"][3].cpu().numpy()
                    same = bool(np.array_equal(ca, cb))
                    for k in (0, 1, 2):
                        xa, xb = out["a"][k].cpu().numpy(), out["b"][k].cpu().numpy()
                        same = same and all(xa[b * n: b * n + ca[b, 0]].tobytes() == xb[b * n: b * n + ca[b, 0]].tobytes() for b in range(B))
                    open_same = bool(np.array_equal(out["a_open"][3].cpu().numpy(), out["c"][3].cpu().numpy()) and
                                     out["a_open"][0].cpu().numpy().tobytes() == out["c"][0].cpu().numpy().tobytes())
                    row = dict(B=B, n=n, dim=dim, gate=a.gate, order=order, variant=variant, tiles_skipped=round(skipped, 4),
                               matches_mean=float(ca[:, 0].mean()), blind_matches_mean=float(out["c"][3].cpu().numpy()[:, 0].mean()), same=same,
                               open_gate_equals_unguided=open_same)
                    for k, v in t.items():
                        row[k + "_us_per_problem"] = [round(float(f(v)) / B, 3) for f in (np.min, np.median, np.max)]
                    row["a_median_below_b_min"] = bool(row["a_us_per_problem"][1] < row["b_us_per_problem"][0])
                    row["open_gate_overhead"] = round(row["a_open_us_per_problem"][1] / row["c_us_per_problem"][1] - 1, 4)
                    if parent:  # the unguided kernel of the two libraries: do the ranges of the rounds overlap?
                        c, cp = row["c_us_per_problem"], row["c_parent_us_per_problem"]
                        row["c_within_spread"] = bool(c[0] <= cp[2] and cp[0] <= c[2])
                        row["c_parent_same"] = bool(out["c_parent"][0].cpu().numpy().tobytes() == out["c"][0].cpu().numpy().tobytes())
                    rows.append(row)
                    lines.append(json.dumps(row))
                    print(lines[-1], flush=True)
    finally:
        reg.close()
        reg_c.close()
        if parent:
            parent.close()
    keys = ["a", "a_open", "b", "c"] + (["c_parent"] if parent else [])
    fmt = lambda v: f"{v[0]:>7.2f} {v[1]:>7.2f} {v[2]:>7.2f}"  # noqa: E731
    lines.append("")
    lines.append(f"{'B':>5} {'order':>7} {'variant':>12} {'skipped':>8} | us per problem, min median max: " + "  ".join(f"{'(' + k + ')':>23}" for k in keys) + "  same  a<b")
    for r in rows:
        lines.append(f"{r['B']:>5} {r['order']:>7} {r['variant']:>12} {r['tiles_skipped']:>8.3f} | {'':>31} " +
                     "  ".join(fmt(r[k + '_us_per_problem']) for k in keys) + f"  {r['same']}  {r['a_median_below_b_min']}")
    print("\n".join(lines[len(rows):]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
