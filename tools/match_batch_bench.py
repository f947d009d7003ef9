#!/usr/bin/env python3
"""What the way from descriptors to poses costs per problem, batched (include/saccot.h, sc_match_batch) and streamed, inputs resident
in HBM.

  python tools/match_batch_bench.py [--batches 16,256,2048] [--n 256] [--dim 33] [--repeats 5] [--warmup 2] [--out profiles/match_batch.txt]

Per B: B problems of n x n keypoints with `dim`-component descriptors (32 distinct seeded scenes, repeated; 30 % of the keypoints
have a partner whose descriptor is a noisy copy), sigma = tau = min_len = 0.05, t_cmp = 0.9, T = 200.  Two variants: knn 1 with
SC_MATCH_MUTUAL (a data-dependent count), and knn 2 (a known one).  Two routes, timed in the same process by a HIP event pair on the
context's stream, `repeats` times after `warmup`, min / median / max in microseconds PER PROBLEM:
  (a) match     one sc_match_batch_device call;
      features  one sc_register_batch_features_device call, descriptors to records;
  (b) match     sc_match_device per problem, streamed on one context;
      features  the same, then the packed batch is laid out — for the mutual variant after the host has read every problem's count,
                which this route cannot avoid —, the matched points are gathered on the device (torch) and ONE
                sc_register_batch_device call registers them.
same: the records of (a) equal those of (b) byte for byte.  Prints one JSON line per (B, variant), then a table; --out receives both.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

DISTINCT = 32


def scene(n, dim, seed, rho=0.3):
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1, 1, size=(n, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    tgt = src @ (q * np.sign(np.linalg.det(q))).T + rng.uniform(-1, 1, size=3) + 0.001 * rng.normal(size=(n, 3))
    k = int(round(rho * n))
    tgt[k:] = rng.uniform(-2, 2, size=(n - k, 3))
    fsrc = rng.normal(size=(n, dim))
    ftgt = fsrc + 0.05 * rng.normal(size=(n, dim))
    ftgt[k:] = rng.normal(size=(n - k, dim))
    perm = rng.permutation(n)
    return [np.ascontiguousarray(x, np.float32) for x in (src, fsrc, tgt[perm], ftgt[perm])]


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
    ap.add_argument("--batches", default="16,256,2048")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--dim", type=int, default=33)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_batch.txt"))
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    n, dim = a.n, a.dim
    p = pkg.make_params(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05, max_triangles=200)
    scenes = [scene(n, dim, 9000 + k) for k in range(DISTINCT)]
    reg = pkg.Registrar(0)
    stream = torch.cuda.Stream(device=dev)
    reg.set_stream(stream.cuda_stream)
    rows, lines = [], []
    try:
        for B in (int(x) for x in a.batches.split(",")):
            pack = [np.concatenate([scenes[b % DISTINCT][k] for b in range(B)]) for k in range(4)]
            d_src, d_fsrc, d_tgt, d_ftgt = (torch.from_numpy(x).to(dev) for x in pack)
            off = (np.arange(B + 1, dtype=np.uint64) * n).astype(np.uint32)
            for variant, mkw in (("knn1_mutual", dict(knn=1, mutual=True)), ("knn2", dict(knn=2))):
                knn = mkw["knn"]
                mp = pkg.api.make_match_params(dim, **mkw)
                slots = B * n * knn
                d_corr = torch.zeros((slots, 2), dtype=torch.int32, device=dev)
                d_d2 = torch.zeros(slots, dtype=torch.float32, device=dev)
                d_count = torch.zeros((B, 2), dtype=torch.int32, device=dev)
                d_res = torch.zeros(B * 80, dtype=torch.uint8, device=dev)
                d_mask = torch.zeros(slots, dtype=torch.uint8, device=dev)
                d_res_b = torch.zeros(B * 80, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()

                def a_match():
                    reg.match_batch_device(d_fsrc.data_ptr(), off, d_ftgt.data_ptr(), off, mp, d_corr.data_ptr(), d_d2.data_ptr(), d_count.data_ptr())

                def a_features():
                    reg.register_batch_features_device(d_src.data_ptr(), d_fsrc.data_ptr(), off, d_tgt.data_ptr(), d_ftgt.data_ptr(), off, mp, p,
                                                       d_res.data_ptr(), d_corr.data_ptr(), d_d2.data_ptr(), d_count.data_ptr(), d_mask.data_ptr())

                def b_match():
                    for b in range(B):
                        reg.match_device(d_fsrc.data_ptr() + b * n * dim * 4, n, d_ftgt.data_ptr() + b * n * dim * 4, n, mp,
                                         d_corr.data_ptr() + b * n * knn * 8, d_d2.data_ptr() + b * n * knn * 4, d_count.data_ptr() + b * 8)

                def b_features():
                    with torch.cuda.stream(stream):
                        counts = []
                        for b in range(B):
                            reg.match_device(d_fsrc.data_ptr() + b * n * dim * 4, n, d_ftgt.data_ptr() + b * n * dim * 4, n, mp,
                                             d_corr.data_ptr() + b * n * knn * 8, d_d2.data_ptr() + b * n * knn * 4, d_count.data_ptr() + b * 8)
                            counts.append(int(d_count[b, 0].item()) if knn == 1 else n * knn)  # mutual: the host read of this count
                        cnt = np.array(counts, np.int64)
                        keep = cnt >= 3  # (sc_register_batch refuses smaller problems: the caller drops them)
                        boff = np.concatenate([[0], np.cumsum(cnt[keep])]).astype(np.uint32)
                        idx = np.concatenate([np.arange(c) + b * n * knn for b, c in enumerate(cnt) if c >= 3])
                        base = np.concatenate([np.full(c, b * n) for b, c in enumerate(cnt) if c >= 3])
                        d_idx, d_base = torch.from_numpy(idx).to(dev), torch.from_numpy(base).to(dev)
                        cv = d_corr[d_idx].long()
                        gs, gt = d_src[cv[:, 0] + d_base].contiguous(), d_tgt[cv[:, 1] + d_base].contiguous()
                        d_m = torch.empty(int(boff[-1]), dtype=torch.uint8, device=dev)
                        reg.register_batch_device(gs.data_ptr(), gt.data_ptr(), boff, p, d_res_b.data_ptr(), d_m.data_ptr())
                        b_features.keep = keep
                        b_features.live = (gs, gt, d_m, d_idx, d_base)  # (alive until the stream has passed them)

                t = {}
                t["a_match"] = timed(torch, stream, a_match, a.warmup, a.repeats)
                t["a_features"] = timed(torch, stream, a_features, a.warmup, a.repeats)
                ra = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE).copy()
                na = d_count.cpu().numpy()[:, 0].copy()
                t["b_match"] = timed(torch, stream, b_match, a.warmup, a.repeats)
                t["b_features"] = timed(torch, stream, b_features, a.warmup, a.repeats)
                torch.cuda.synchronize()
                keep = b_features.keep
                rb = np.frombuffer(d_res_b.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE)[: int(keep.sum())]
                same = bool(ra[keep].tobytes() == rb.tobytes())
                row = dict(B=B, n=n, dim=dim, variant=variant, matches_mean=float(na.mean()), statuses_ok=int((ra["status"] == 0).sum()), same=same)
                for k, v in t.items():
                    row[k + "_us_per_problem"] = [round(float(f(v)) / B, 3) for f in (np.min, np.median, np.max)]
                row["a_median_below_b_min"] = bool(row["a_features_us_per_problem"][1] < row["b_features_us_per_problem"][0] and
                                                   row["a_match_us_per_problem"][1] < row["b_match_us_per_problem"][0])
                rows.append(row)
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
    finally:
        reg.close()
    fmt = lambda v: f"{v[0]:>8.2f} {v[1]:>8.2f} {v[2]:>8.2f}"  # noqa: E731
    lines.append("")
    lines.append(f"{'B':>5} {'variant':>12} | us per problem, min median max: {'(a) match':>22} {'(a) features':>26} {'(b) match':>26} {'(b) features':>26}  same")
    for r in rows:
        lines.append(f"{r['B']:>5} {r['variant']:>12} | {'':>31} " + "  ".join(fmt(r[k + '_us_per_problem']) for k in ("a_match", "a_features", "b_match", "b_features")) + f"  {r['same']}")
    print("\n".join(lines[len(rows):]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
