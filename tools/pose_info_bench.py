#!/usr/bin/env python3
"""What the information matrices of a batch's poses cost (include/saccot.h, sc_pose_info_batch), inputs resident in HBM.

  python tools/pose_info_bench.py [--sizes 128,256,512] [--batches 64,1024,4096] [--repeats 20] [--warmup 2]
                                  [--out profiles/pose_info.txt]

Per (n, B): tools/polish_batch_bench.py's scenes — B problems of n correspondences (32 distinct seeded scenes, repeated; rho = 0.3),
sigma = min_len = 0.05, t_cmp = 0.9, T = 2000, tau = 0.02, max_iter = 16.  Device time by a HIP event pair on the context's stream,
median of `repeats` after `warmup`, in microseconds:
  register   one sc_register_batch_device call;
  polish     one sc_polish_batch_device call on its records;
  info       one sc_pose_info_batch_device call on the polished records (stride 64).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_info.txt"))
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    p = pkg.make_params(sigma=0.05, t_cmp=0.9, tau=0.02, min_len=0.05, max_triangles=2000)
    q = pkg.make_polish_params(candidates=1, max_iter=16)
    reg = pkg.Registrar(0)
    stream = torch.cuda.Stream(device=dev)
    reg.set_stream(stream.cuda_stream)
    rows, lines = [], []
    try:
        for n in (int(x) for x in a.sizes.split(",")):
            scenes = [pkg.synth.make_scene(n, 0.3, 1.0, 0.05, 9000 + n + k) for k in range(DISTINCT)]
            for B in (int(x) for x in a.batches.split(",")):
                src = np.concatenate([scenes[b % DISTINCT].src for b in range(B)]).astype(np.float32)
                tgt = np.concatenate([scenes[b % DISTINCT].tgt for b in range(B)]).astype(np.float32)
                d_src, d_tgt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
                off = (np.arange(B + 1, dtype=np.uint64) * n).astype(np.uint32)
                d_res = torch.zeros(B * 80, dtype=torch.uint8, device=dev)
                d_pol = torch.zeros(B * 64, dtype=torch.uint8, device=dev)
                d_mask = torch.zeros(B * n, dtype=torch.uint8, device=dev)
                d_info = torch.zeros(B * 320, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()

                def register():
                    reg.register_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_res.data_ptr(), d_mask.data_ptr())

                def polish():
                    reg.polish_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, q, d_res.data_ptr(), d_pol.data_ptr(), d_mask.data_ptr())

                def info():
                    reg.pose_info_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, d_pol.data_ptr(), 64, d_info.data_ptr())

                t_reg = timed(torch, stream, register, a.warmup, a.repeats)
                t_pol = timed(torch, stream, polish, a.warmup, a.repeats)
                t_inf = timed(torch, stream, info, a.warmup, a.repeats)
                torch.cuda.synchronize()
                pol = np.frombuffer(d_pol.cpu().numpy().tobytes(), pkg.api.POLISH_BATCH_RESULT_DTYPE)
                rec = np.frombuffer(d_info.cpu().numpy().tobytes(), pkg.POSE_INFO_RESULT_DTYPE)
                med = lambda v: float(np.median(v))  # noqa: E731
                row = dict(n=n, B=B, statuses_ok=int((rec["status"] == 0).sum()), inliers_mean=round(float(rec["inliers"].mean()), 1),
                           counts_agree=bool(np.array_equal(rec["inliers"], pol["score"])), register_us=round(med(t_reg), 1),
                           polish_us=round(med(t_pol), 1), info_us=round(med(t_inf), 1),
                           info_us_min_max=[round(float(min(t_inf)), 1), round(float(max(t_inf)), 1)],
                           info_over_polish=round(med(t_inf) / med(t_pol), 4))
                rows.append(row)
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
    finally:
        reg.close()
    lines.append("")
    lines.append(f"{'n':>4} {'B':>5} | {'register us':>12} {'polish us':>10} {'info us':>9} {'info/polish':>12} {'inliers mean':>13}  counts agree")
    for r in rows:
        lines.append(f"{r['n']:>4} {r['B']:>5} | {r['register_us']:>12.1f} {r['polish_us']:>10.1f} {r['info_us']:>9.1f} {r['info_over_polish']:>12.4f} "
                     f"{r['inliers_mean']:>13.1f}  {r['counts_agree']}")
    print("\n".join(lines[len(rows):]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
