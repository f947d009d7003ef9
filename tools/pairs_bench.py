#!/usr/bin/env python3
"""What registering listed pairs of shared keypoint sets costs (include/saccot.h, sc_match_pairs), against the way a caller had
before: expand the table into packed arrays on the device, then the packed entries.  Inputs resident in HBM.

  python tools/pairs_bench.py [--sets 64] [--n 256] [--dim 32] [--random 256] [--repeats 7] [--warmup 3] [--out profiles/pairs.txt]

A table of `sets` sets of n keypoints with `dim`-component descriptors: set s is a rigidly moved, noisy copy of one base cloud (30 %
of its keypoints keep the base's descriptor, noisily), so any two sets register.  knn 1 with SC_MATCH_MUTUAL, sigma = tau = min_len
= 0.05, t_cmp = 0.9, T = 200.  Two lists — all sets * (sets - 1) / 2 pairs, and `random` random pairs — each in three orders: as
generated, sorted by target set, shuffled (is the L2 reuse of a shared set visible?).  Timed in the same process by a HIP event pair
on the context's stream, `repeats` times after `warmup`, min / median / max in microseconds PER CALL:
  pairs_match     one sc_match_pairs_device call;
  pairs_features  one sc_register_pairs_features_device call;
  expand          the parent's expansion alone: four device-side row gathers (torch.index_select into preallocated arrays; the row
                  indices already on the device, which favours this route);
  packed_match    one sc_match_batch_device call on the expanded arrays;
  packed_features one sc_register_batch_features_device call on them.
same: the records, count pairs and the specified slot entries of the two routes are equal byte for byte.  Prints one JSON line per
(list, order), then a table; --out receives both.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def make_table(sets, n, dim, rho=0.3):
    rng = np.random.default_rng(64)
    base_p = rng.uniform(-1, 1, size=(n, 3)); base_f = rng.normal(size=(n, dim))
    k = int(round(rho * n))
    pts, feat = [], []
    for s in range(sets):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        p = base_p @ (q * np.sign(np.linalg.det(q))).T + rng.uniform(-1, 1, size=3) + 0.001 * rng.normal(size=(n, 3))
        f = base_f + 0.05 * rng.normal(size=(n, dim))
        p[k:] = rng.uniform(-2, 2, size=(n - k, 3)); f[k:] = rng.normal(size=(n - k, dim))
        perm = rng.permutation(n)
        pts.append(p[perm]); feat.append(f[perm])
    return np.ascontiguousarray(np.concatenate(pts), np.float32), np.ascontiguousarray(np.concatenate(feat), np.float32)


def timed(torch, stream, fn, warmup, repeats):
    out = []
    for it in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--random", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs.txt"))
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    S, n, dim = a.sets, a.n, a.dim
    p = pkg.make_params(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05, max_triangles=200)
    mp = pkg.api.make_match_params(dim, knn=1, mutual=True)
    pts, feat = make_table(S, n, dim)
    set_off = (np.arange(S + 1, dtype=np.uint64) * n).astype(np.uint32)
    d_pts, d_feat = torch.from_numpy(pts).to(dev), torch.from_numpy(feat).to(dev)
    rng = np.random.default_rng(7)
    every = np.array([(i, j) for i in range(S) for j in range(i + 1, S)], np.uint32)
    first = rng.integers(0, S, size=a.random)
    other = (first + 1 + rng.integers(0, S - 1, size=a.random)) % S  # (no self pair: all of its keypoints match, a long registration)
    lists = {"all": every, "random": np.stack([first, other], axis=1).astype(np.uint32)}
    reg = pkg.Registrar(0)
    stream = torch.cuda.Stream(device=dev)
    reg.set_stream(stream.cuda_stream)
    rows, lines = [], []
    try:
        for name, base in lists.items():
            orders = {"as generated": base, "by target": base[np.argsort(base[:, 1], kind="stable")], "shuffled": base[rng.permutation(len(base))]}
            for order, pairs in orders.items():
                P = len(pairs)
                slots = P * n
                off = (np.arange(P + 1, dtype=np.uint64) * n).astype(np.uint32)
                rows_of = lambda sets_: (sets_.astype(np.int64)[:, None] * n + np.arange(n)[None, :]).reshape(-1)  # noqa: E731
                d_is, d_it = torch.from_numpy(rows_of(pairs[:, 0])).to(dev), torch.from_numpy(rows_of(pairs[:, 1])).to(dev)
                x = dict(ps=torch.empty((slots, 3), dtype=torch.float32, device=dev), pt=torch.empty((slots, 3), dtype=torch.float32, device=dev),
                         fs=torch.empty((slots, dim), dtype=torch.float32, device=dev), ft=torch.empty((slots, dim), dtype=torch.float32, device=dev))
                out = [dict(corr=torch.zeros((slots, 2), dtype=torch.int32, device=dev), d2=torch.zeros(slots, dtype=torch.float32, device=dev),
                            count=torch.zeros((P, 2), dtype=torch.int32, device=dev), res=torch.zeros(P * 80, dtype=torch.uint8, device=dev),
                            mask=torch.zeros(slots, dtype=torch.uint8, device=dev)) for _ in range(2)]
                torch.cuda.synchronize()
                A, B = out

                def pairs_match():
                    reg.match_pairs_device(d_feat.data_ptr(), set_off, pairs, mp, A["corr"].data_ptr(), A["d2"].data_ptr(), A["count"].data_ptr())

                def pairs_features():
                    reg.register_pairs_features_device(d_pts.data_ptr(), d_feat.data_ptr(), set_off, pairs, mp, p, A["res"].data_ptr(),
                                                       A["corr"].data_ptr(), A["d2"].data_ptr(), A["count"].data_ptr(), A["mask"].data_ptr())

                def expand():
                    with torch.cuda.stream(stream):
                        torch.index_select(d_pts, 0, d_is, out=x["ps"]); torch.index_select(d_feat, 0, d_is, out=x["fs"])
                        torch.index_select(d_pts, 0, d_it, out=x["pt"]); torch.index_select(d_feat, 0, d_it, out=x["ft"])

                def packed_match():
                    reg.match_batch_device(x["fs"].data_ptr(), off, x["ft"].data_ptr(), off, mp, B["corr"].data_ptr(), B["d2"].data_ptr(),
                                           B["count"].data_ptr())

                def packed_features():
                    reg.register_batch_features_device(x["ps"].data_ptr(), x["fs"].data_ptr(), off, x["pt"].data_ptr(), x["ft"].data_ptr(), off, mp, p,
                                                       B["res"].data_ptr(), B["corr"].data_ptr(), B["d2"].data_ptr(), B["count"].data_ptr(),
                                                       B["mask"].data_ptr())

                t = {}
                for fn in (expand, pairs_match, packed_match, pairs_features, packed_features):
                    t[fn.__name__] = timed(torch, stream, fn, a.warmup, a.repeats)
                torch.cuda.synchronize()
                h = [{k: v.cpu().numpy() for k, v in o.items()} for o in out]
                cnt = h[0]["count"]
                same = all(h[0][k].tobytes() == h[1][k].tobytes() for k in ("count", "res"))
                for k in ("corr", "d2", "mask"):
                    same = same and all(h[0][k][b * n: b * n + cnt[b, 0]].tobytes() == h[1][k][b * n: b * n + cnt[b, 0]].tobytes() for b in range(P))
                res = np.frombuffer(h[0]["res"].tobytes(), pkg.BATCH_RESULT_DTYPE)
                row = dict(list=name, order=order, pairs=P, sets=S, n=n, dim=dim, matches_mean=float(cnt[:, 0].mean()),
                           statuses_ok=int((res["status"] == 0).sum()), same=bool(same),
                           table_MB=round((pts.nbytes + feat.nbytes) / 1e6, 2), expanded_MB=round(sum(v.numel() * 4 for v in x.values()) / 1e6, 2))
                for k, v in t.items():
                    row[k + "_us"] = [round(float(f(v)), 1) for f in (np.min, np.median, np.max)]
                rows.append(row)
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
                del x, out, A, B
    finally:
        reg.close()
    keys = ("pairs_match", "packed_match", "pairs_features", "packed_features", "expand")
    fmt = lambda v: f"{v[0]:>9.1f} {v[1]:>9.1f} {v[2]:>9.1f}"  # noqa: E731
    lines.append("")
    lines.append(f"{'list':>7} {'order':>13} {'pairs':>6} | us per call, min median max: " + "  ".join(f"{k:>29}" for k in keys) + "  same")
    for r in rows:
        lines.append(f"{r['list']:>7} {r['order']:>13} {r['pairs']:>6} | {'':>28} " + "  ".join(fmt(r[k + '_us']) for k in keys) + f"  {r['same']}")
    print("\n".join(lines[len(rows):]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
