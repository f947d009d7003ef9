#!/usr/bin/env python3
"""What further motions cost a batch member (include/saccot.h, sc_register_instances_batch), inputs resident in HBM.

  python tools/instances_batch_bench.py [--sizes 128,256,512] [--batches 64,1024,4096] [--repeats 20] [--warmup 2] [--single-max 256]
                                        [--out profiles/instances_batch.txt]

Per (n, B): B problems of n correspondences (32 distinct seeded two-motion scenes, repeated: 0.18 n and 0.12 n correspondences on the
two motions, rho = 0.3 split 0.6 / 0.4), sigma = tau = min_len = 0.05, t_cmp = 0.9, T = 2000, max_instances = 4, min_score = 4.  Device time by a HIP event
pair on the context's stream, median of `repeats` after `warmup`, in microseconds:
  instances  one sc_register_instances_batch_device call;
  register   one sc_register_batch_device call on the same problems (the frames alone);
  twice      two successive sc_register_batch_device calls: the lower bound of the route "compact the unclaimed correspondences on
             the host and call the batch again" (the second call here is as large as the first and nothing crosses the host);
  single     the same problems one at a time through sc_register_instances (host arrays) — min(B, --single-max) of them, scaled to
             B (the route is linear in B: one frame and its rounds per problem).
same: every motion of the batch (Rt, score), the labels and the count equal those of the single route bit for bit, over the problems
the single route ran — asserted, not only reported.
Prints one JSON line per (n, B), then a table; --out receives both.
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
MAX_INSTANCES, MIN_SCORE = 4, 4


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
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--single-max", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instances_batch.txt"))
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    kw = dict(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05, max_triangles=2000)
    p = pkg.make_params(**kw)
    p_single = pkg.make_params(**kw, flags=pkg.SC_FLAG_EXACT_TOTAL)
    reg = pkg.Registrar(0)
    stream = torch.cuda.Stream(device=dev)
    reg.set_stream(stream.cuda_stream)
    rows, lines = [], []
    try:
        for n in (int(x) for x in a.sizes.split(",")):
            scenes = [pkg.synth.make_scene_motions(n, [0.18, 0.12], 1.0, 0.05, 9500 + n + k) for k in range(DISTINCT)]
            for B in (int(x) for x in a.batches.split(",")):
                src = np.concatenate([scenes[b % DISTINCT].src for b in range(B)]).astype(np.float32)
                tgt = np.concatenate([scenes[b % DISTINCT].tgt for b in range(B)]).astype(np.float32)
                d_src, d_tgt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
                off = (np.arange(B + 1, dtype=np.uint64) * n).astype(np.uint32)
                d_res = torch.zeros(MAX_INSTANCES * B * 80, dtype=torch.uint8, device=dev)
                d_label = torch.zeros(B * n, dtype=torch.int32, device=dev)
                d_nfound = torch.zeros(B, dtype=torch.int32, device=dev)
                d_mask = torch.zeros(B * n, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()

                def instances():
                    reg.register_instances_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, MAX_INSTANCES, MIN_SCORE, d_res.data_ptr(),
                                                        d_label.data_ptr(), d_nfound.data_ptr())

                def register():
                    reg.register_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_res.data_ptr(), d_mask.data_ptr())

                def twice():
                    register()
                    register()

                ns = min(B, a.single_max)
                single_out = []

                def single():
                    single_out.clear()
                    for b in range(ns):
                        single_out.append(reg.register_instances(src[b * n: (b + 1) * n], tgt[b * n: (b + 1) * n], max_instances=MAX_INSTANCES,
                                                                 min_score=MIN_SCORE, params=p_single))

                t_reg = timed(torch, stream, register, a.warmup, a.repeats)
                t_two = timed(torch, stream, twice, a.warmup, a.repeats)
                t_one = timed(torch, stream, single, 1, max(3, a.repeats // 4))
                t_ins = timed(torch, stream, instances, a.warmup, a.repeats)  # last: d_res holds its planes
                torch.cuda.synchronize()
                recs = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.BATCH_RESULT_DTYPE).reshape(MAX_INSTANCES, B)
                label, nfound = d_label.cpu().numpy().reshape(B, n), d_nfound.cpu().numpy()
                for b in range(ns):
                    o, k = single_out[b], int(nfound[b])
                    assert len(o["score"]) == k and np.array_equal(o["score"], recs[:k, b]["best_count"]), (n, B, b)
                    assert np.array_equal(o["Rt"].view(np.uint32), recs[:k, b]["Rt"].view(np.uint32)), (n, B, b)
                    assert np.array_equal(o["label"], label[b]), (n, B, b)
                med = lambda v: float(np.median(v))  # noqa: E731
                row = dict(n=n, B=B, found_mean=round(float(nfound.mean()), 2), found_hist=np.bincount(nfound, minlength=MAX_INSTANCES + 1).tolist(),
                           triangles_mean=float(np.mean(recs[0]["tri_total"].astype(np.float64))),
                           instances_us=round(med(t_ins), 1), instances_us_min_max=[round(float(min(t_ins)), 1), round(float(max(t_ins)), 1)],
                           register_us=round(med(t_reg), 1), twice_us=round(med(t_two), 1), single_us=round(med(t_one) * B / ns, 1), single_ran=ns,
                           instances_over_register=round(med(t_ins) / med(t_reg), 3), instances_over_twice=round(med(t_ins) / med(t_two), 3),
                           same=True)
                rows.append(row)
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
    finally:
        reg.close()
    lines.append("")
    lines.append(f"{'n':>4} {'B':>5} | {'instances us':>13} {'register us':>12} {'twice us':>10} {'single us (scaled)':>19} {'inst/reg':>9} {'inst/twice':>11} "
                 f"{'found mean':>11}  same")
    for r in rows:
        lines.append(f"{r['n']:>4} {r['B']:>5} | {r['instances_us']:>13.1f} {r['register_us']:>12.1f} {r['twice_us']:>10.1f} {r['single_us']:>19.1f} "
                     f"{r['instances_over_register']:>9.3f} {r['instances_over_twice']:>11.3f} {r['found_mean']:>11.2f}  {r['same']}")
    print("\n".join(lines[len(rows):]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
