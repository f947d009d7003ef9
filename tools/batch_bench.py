#!/usr/bin/env python3
"""What a small problem costs in a batch (include/saccot.h, sc_register_batch) and streamed, inputs resident in HBM.

  python tools/batch_bench.py [--sizes 128,256,512] [--batches 64,256,1024,4096] [--steps 20] [--warmup 3] [--T 2000] [--rho 0.3]

Per (n, B): B problems of n correspondences (32 distinct seeded scenes, repeated), sigma = tau = min_len = 0.05, t_cmp = 0.9.
  batch_us_per_problem     device time of ONE sc_register_batch_device call over B: a HIP event pair around the call on the context's
                           stream, median of `steps` after `warmup` calls;
  streamed2_us_per_problem the same problems one sc_register_device_async / sc_wait at a time, two contexts on ONE stream (the next
                           frame is enqueued while the last one runs): host clock around the loop, ending in a device synchronise;
  streamed4_us_per_problem four contexts on four streams, as bench.py's calls_in_flight does.
The streamed loops run over the first min(B, 256) problems (their time per problem does not depend on B), after a warm-up round over
the same problems, best of three.  same_winner: every streamed (status, best_rank, best_count) equals the batch's record.
Prints one JSON line per (n, B), then a table.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

DISTINCT = 32


def streamed(pkg, torch, regs, d_src, d_tgt, off, n, p, count, outs):
    """`count` problems through len(regs) contexts, one call outstanding on each -> (seconds, [(status, rank, count)])"""
    nfl = len(regs)
    got = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(count + nfl - 1):
        if k < count:
            i = k % nfl
            regs[i].register_device_async(d_src.data_ptr() + int(off[k]) * 12, d_tgt.data_ptr() + int(off[k]) * 12, n, p,
                                          outs[i][0].data_ptr(), outs[i][1].data_ptr())
        if k >= nfl - 1:
            rc, st = regs[(k - nfl + 1) % nfl].wait()
            got.append((rc, st["best_rank"], st["best_count"]))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--batches", default="64,256,1024,4096")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--rho", type=float, default=0.3)
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    kw = dict(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05, max_triangles=a.T)
    p = pkg.make_params(**kw)
    rows = []
    batch_reg = pkg.Registrar(0)
    stream = torch.cuda.Stream(device=dev)
    batch_reg.set_stream(stream.cuda_stream)
    two = [pkg.Registrar(0) for _ in range(2)]
    for g in two:
        g.set_stream(stream.cuda_stream)
    four = [pkg.Registrar(0) for _ in range(4)]
    four_streams = [torch.cuda.Stream(device=dev) for _ in range(4)]
    for g, s in zip(four, four_streams):
        g.set_stream(s.cuda_stream)
    try:
        for n in (int(x) for x in a.sizes.split(",")):
            scenes = [pkg.synth.make_scene(n, a.rho, 1.0, 0.05, 9000 + k) for k in range(DISTINCT)]
            outs = [(torch.zeros(12, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)) for _ in range(4)]
            for B in (int(x) for x in a.batches.split(",")):
                src = np.concatenate([scenes[b % DISTINCT].src for b in range(B)])
                tgt = np.concatenate([scenes[b % DISTINCT].tgt for b in range(B)])
                off = (np.arange(B + 1, dtype=np.uint64) * n).astype(np.uint32)
                d_src, d_tgt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
                d_res = torch.zeros(B * 80, dtype=torch.uint8, device=dev)
                d_mask = torch.zeros(B * n, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                times = []
                for it in range(a.warmup + a.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    batch_reg.register_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_res.data_ptr(), d_mask.data_ptr())
                    e1.record(stream)
                    e1.synchronize()
                    if it >= a.warmup:
                        times.append(e0.elapsed_time(e1) * 1e3)
                recs = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE)
                want = [(int(r["status"]), int(r["best_rank"]), int(r["best_count"])) for r in recs]
                count = min(B, 256)
                res = {}
                for name, regs in (("streamed2", two), ("streamed4", four)):
                    streamed(pkg, torch, regs, d_src, d_tgt, off, n, p, count, outs)  # warm-up: every context has seen the shape
                    best, same = None, True
                    for _ in range(3):
                        sec, got = streamed(pkg, torch, regs, d_src, d_tgt, off, n, p, count, outs)
                        best = sec if best is None or sec < best else best
                        same = same and got == want[:count]
                    res[name + "_us_per_problem"] = round(best / count * 1e6, 2)
                    res[name + "_same_winner"] = bool(same)
                row = dict(n=n, B=B, T=a.T, rho=a.rho, triangles_mean=float(np.mean(recs["tri_total"].astype(np.float64))),
                           batch_us_per_call=round(float(np.median(times)), 1), batch_us_per_problem=round(float(np.median(times)) / B, 3),
                           statuses_ok=int((recs["status"] == 0).sum()), **res)
                row["ratio_best_streamed_over_batch"] = round(min(res["streamed2_us_per_problem"], res["streamed4_us_per_problem"]) /
                                                              row["batch_us_per_problem"], 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
    finally:
        for g in [batch_reg] + two + four:
            g.close()
    print(f"\n{'n':>4} {'B':>5} {'triangles':>10} {'batch us/call':>14} {'batch us/problem':>17} {'streamed x2':>12} {'streamed x4':>12} {'ratio':>6}")
    for r in rows:
        print(f"{r['n']:>4} {r['B']:>5} {r['triangles_mean']:>10.0f} {r['batch_us_per_call']:>14.1f} {r['batch_us_per_problem']:>17.3f} "
              f"{r['streamed2_us_per_problem']:>12.2f} {r['streamed4_us_per_problem']:>12.2f} {r['ratio_best_streamed_over_batch']:>6.1f}")


if __name__ == "__main__":
    main()
