#!/usr/bin/env python3
"""What descriptor matching costs (include/saccot.h, sc_match): C2-shaped input (5000 x 5300 descriptors), resident in HBM.

  python tools/match_bench.py [--steps 50] [--warmup 5] [--config C2] [--dims 33,352]

Per descriptor length D, k = 1, plain and mutual:
  match_us       median device time of sc_match_device (memset + distance + finish launches), HIP events on the context's stream;
  floor_fraction the arithmetic floor 3 D ns nt lane-operations at half the fp32 vector peak (157.3 / 2 TFLOP/s) over match_us;
  cdist_argmin_us  torch.cdist(a, b).argmin(1) on the same resident tensors in the same run — what a caller does today.  A time
                 only: its rounding and ties are not the canonical ones.
Then, at the first D, host arrays in and out:
  register_features_wall_us   against sc_match + a gather of the matched points on the host + sc_register.
Prints one JSON line.  The frame the matcher stands in front of is bench.py's ms_per_step.
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

PEAK_LANE_OPS = 157.3e12 / 2  # fp32 vector peak in FLOP/s counts a fused multiply-add as two; sub, mul, add are one lane-operation each


def med(x):
    return round(float(np.median(x)), 2)


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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="C2")
    ap.add_argument("--dims", default="33,352")
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    cfg = pkg.synth.CONFIGS[a.config]
    dims = [int(x) for x in a.dims.split(",")]
    dev = torch.device("cuda:0")
    out = dict(config=a.config, ns=cfg.n, nt=cfg.n + 300, steps=a.steps, warmup=a.warmup, by_dim={})
    r = pkg.Registrar(0)
    try:
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        for D in dims:
            sc = pkg.synth.make_feature_scene(cfg, 300, D, 1.0)
            ns, nt = sc.fsrc.shape[0], sc.ftgt.shape[0]
            da, db = torch.from_numpy(sc.fsrc).to(dev), torch.from_numpy(sc.ftgt).to(dev)
            d_corr = torch.zeros((ns, 2), dtype=torch.int32, device=dev)
            d_d2 = torch.zeros(ns, dtype=torch.float32, device=dev)
            d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
            floor_us = 3.0 * D * ns * nt / PEAK_LANE_OPS * 1e6
            row = dict(floor_us=round(floor_us, 2))
            for name, mutual in (("plain", False), ("mutual", True)):
                mp = pkg.api.make_match_params(D, mutual=mutual)
                us = events_us(torch, lambda: r.match_device(da.data_ptr(), ns, db.data_ptr(), nt, mp, d_corr.data_ptr(), d_d2.data_ptr(),
                                                             d_cnt.data_ptr()), a.steps, a.warmup)
                n, flag = d_cnt.cpu().tolist()
                assert flag == 0
                row[name] = dict(match_us=med(us), min_us=round(min(us), 2), floor_fraction=round(floor_us / float(np.median(us)), 3), n=n)
            nn = []
            us = events_us(torch, lambda: nn.append(torch.cdist(da, db).argmin(1)), a.steps, a.warmup)
            agree = float((nn[-1].cpu().numpy() == r.match(sc.fsrc, sc.ftgt)["corr"][:, 1]).mean())
            row["cdist_argmin_us"] = med(us)
            row["cdist_argmin_agrees_with_canonical"] = round(agree, 5)  # (information: torch's rounding and ties are its own)
            out["by_dim"][str(D)] = row
        # descriptors in, (R, t) out — host arrays, wall clock
        D = dims[0]
        sc = pkg.synth.make_feature_scene(cfg, 300, D, 1.0)
        p = pkg.make_params(**cfg.params())
        r.set_stream(None)
        for name, mutual in (("plain", False), ("mutual", True)):
            one, parts = [], []
            for it in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                res = r.register_features(sc.src_pts, sc.fsrc, sc.tgt_pts, sc.ftgt, params=p, mutual=mutual)
                t1 = time.perf_counter()
                assert res["status"] == 0
                if it >= a.warmup:
                    one.append((t1 - t0) * 1e6)
            for it in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                m = r.match(sc.fsrc, sc.ftgt, mutual=mutual)
                src = np.ascontiguousarray(sc.src_pts[m["corr"][:, 0]])
                tgt = np.ascontiguousarray(sc.tgt_pts[m["corr"][:, 1]])
                g = r.register(src, tgt, params=p)
                t1 = time.perf_counter()
                assert g["status"] == 0 and g["stats"]["best_count"] == res["stats"]["best_count"]
                if it >= a.warmup:
                    parts.append((t1 - t0) * 1e6)
            out["register_features_" + name] = dict(D=D, n=res["n"], winner_inliers=res["stats"]["best_count"], register_features_wall_us=med(one),
                                                    match_gather_register_wall_us=med(parts))
    finally:
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
