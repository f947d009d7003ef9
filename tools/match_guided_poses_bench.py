#!/usr/bin/env python3
"""What the pose loop of sc_match_guided_poses costs and what one union match saves (include/saccot.h): 5000 x 5300 keypoints with
descriptors of length 33, gate 0.05, resident in HBM, keypoints in random order and in Morton order.

  python tools/match_guided_poses_bench.py [--steps 30] [--warmup 5] [--rounds 3] [--table]

Device time by HIP events around the calls on the context's stream, median over --steps repetitions after --warmup; every figure is
taken --rounds times, the rounds of the things compared alternating, and reported as the median of the rounds' medians with their
spread (max - min): a difference inside the spread is no difference.
  K = 1    sc_match_guided_poses_device with one record beside sc_match_guided_device of the same tree on the same scene: the
           price of the pose loop (the pose read from LDS per cell instead of held in registers).  The outputs are compared.
  K = 4,   a scene of K moved groups (source row i belongs to group i % K, a third of the targets are planted under their group's
  K = 16   pose, the rest is clutter): ONE call under the K records beside K calls of sc_match_guided_device, one per pose, in one
           bracket.  The K calls are not the same operation (K overlapping lists); the figure says what the union costs beside them.
Prints one JSON line; --table also prints the rows as text.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

NS, NT, D, GATE = 5000, 5300, 33, 0.05


def events_us(torch, fn, steps, warmup):
    out = []
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))


def random_pose(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q, rng.standard_normal(3) * 0.5


def scene(K, seed=1):
    """source keypoints in the unit cube in K groups (row i: group i % K), K random poses, the first third of the targets copies of
    source rows under their group's pose (point noise 0.01, descriptor noise 0.3), the rest random points of the cube under a random
    pose of the list; the targets in random order"""
    rng = np.random.default_rng(seed)
    src = rng.random((NS, 3))
    poses = [random_pose(rng) for _ in range(K)]
    which = rng.integers(0, K, NT)
    raw = rng.random((NT, 3))
    tgt = np.stack([raw[j] @ poses[which[j]][0].T + poses[which[j]][1] for j in range(NT)])
    fsrc = rng.standard_normal((NS, D)).astype(np.float32)
    ftgt = rng.standard_normal((NT, D)).astype(np.float32)
    m = NT // 3
    rows = rng.permutation(NS)[:m]
    for c, i in enumerate(rows):
        q, t = poses[i % K]
        tgt[c] = src[i] @ q.T + t + 0.01 * rng.standard_normal(3)
    ftgt[:m] = fsrc[rows] + np.float32(0.3) * rng.standard_normal((m, D)).astype(np.float32)
    perm = rng.permutation(NT)
    Rt = np.stack([np.concatenate([q.ravel(), t]) for q, t in poses]).astype(np.float32)
    return src.astype(np.float32), fsrc, tgt[perm].astype(np.float32), ftgt[perm], Rt


def morton_order(p):
    """rows of p along a Morton curve of 10 bits an axis over p's own bounding box"""
    lo, hi = p.min(axis=0), p.max(axis=0)
    g = np.clip(((p - lo) / np.maximum(hi - lo, 1e-9) * 1024).astype(np.int64), 0, 1023)
    code = np.zeros(len(p), np.int64)
    for b in range(10):
        for c in range(3):
            code |= ((g[:, c] >> b) & 1) << (3 * b + c)
    return np.argsort(code, kind="stable")


def summary(rounds):
    return dict(us=round(float(np.median(rounds)), 2), spread_us=round(float(max(rounds) - min(rounds)), 2), rounds=[round(x, 2) for x in rounds])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    out = dict(ns=NS, nt=NT, dim=D, gate=GATE, steps=a.steps, warmup=a.warmup, rounds=a.rounds, rows=[])
    r = pkg.Registrar(0)
    try:
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        mp, gp = pkg.api.make_match_params(D), pkg.make_guide_params(GATE)
        d_corr = torch.zeros((NS, 2), dtype=torch.int32, device=dev); d_d2 = torch.zeros(NS, dtype=torch.float32, device=dev)
        d_g2 = torch.zeros(NS, dtype=torch.float32, device=dev); d_lab = torch.zeros(NS, dtype=torch.int32, device=dev)
        d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        for K in [int(x) for x in a.ks.split(",")]:
            src, fsrc, tgt, ftgt, Rt = scene(K)
            so, to = morton_order(src), morton_order(tgt)
            for order, arrs in (("random", (src, fsrc, tgt, ftgt)), ("morton", (src[so], fsrc[so], tgt[to], ftgt[to]))):
                d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in arrs]
                d_pose = torch.from_numpy(Rt).to(dev)

                def union():
                    r.match_guided_poses_device(d[0].data_ptr(), d[1].data_ptr(), NS, d[2].data_ptr(), d[3].data_ptr(), NT, mp, gp,
                                                d_pose.data_ptr(), 48, K, d_corr.data_ptr(), d_d2.data_ptr(), d_g2.data_ptr(), d_lab.data_ptr(),
                                                d_cnt.data_ptr())

                def singles():
                    for k in range(K):
                        r.match_guided_device(d[0].data_ptr(), d[1].data_ptr(), NS, d[2].data_ptr(), d[3].data_ptr(), NT, mp, gp,
                                              d_pose.data_ptr() + 48 * k, d_corr.data_ptr(), d_d2.data_ptr(), d_g2.data_ptr(), d_cnt.data_ptr())

                t_union, t_single = [], []
                for _ in range(a.rounds):  # alternating
                    t_single.append(events_us(torch, singles, a.steps, a.warmup))
                    t_union.append(events_us(torch, union, a.steps, a.warmup))
                union(); torch.cuda.synchronize()
                n, flag = d_cnt.cpu().tolist()
                assert flag == 0
                row = dict(K=K, order=order, n=n, poses=summary(t_union), single_calls=summary(t_single),
                           labels=np.bincount(d_lab.cpu().numpy()[:n], minlength=K).tolist())
                if K == 1:  # the same answer as the single-pose entry's
                    got = (d_corr.cpu().numpy()[:n].copy(), d_d2.cpu().numpy()[:n].copy(), d_g2.cpu().numpy()[:n].copy())
                    singles(); torch.cuda.synchronize()
                    assert d_cnt.cpu().tolist() == [n, 0]
                    assert all(x.tobytes() == y.cpu().numpy()[:n].tobytes() for x, y in zip(got, (d_corr, d_d2, d_g2)))
                out["rows"].append(row)
    finally:
        r.close()
    print(json.dumps(out))
    if a.table:
        for row in out["rows"]:
            p, s = row["poses"], row["single_calls"]
            print(f"K {row['K']:>2} {row['order']:>6}: one call under K records {p['us']:9.2f} us (spread {p['spread_us']:6.2f}) | "
                  f"K calls of sc_match_guided_device {s['us']:9.2f} us (spread {s['spread_us']:6.2f}) | ratio {p['us'] / s['us']:5.2f} | n {row['n']}")


if __name__ == "__main__":
    main()
