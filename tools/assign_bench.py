#!/usr/bin/env python3
"""What labelling a frame's correspondences by K poses costs (include/saccot.h, sc_assign_poses), everything resident in HBM.

  python tools/assign_bench.py [--configs C2,C3] [--poses 2,8,64,1024] [--repeats 30] [--warmup 5] [--batch-sizes 128,512]
                               [--batches 64,1024,4096] [--out profiles/assign.txt] [--prepend FILE ...]

The frame form.  Per config (C2: bench.py's shape, n = 5 000; C3: n = 20 000, scored here on one GPU with T = 50 000): the config's
own scene, registered once: the frame every timed call then runs on.  The K poses are the frame's winner with small seeded
translations added (a tenth of tau), every seventh of them a pose far away.  Device time by a HIP event pair on the context's stream,
median of `repeats` after `warmup`, in microseconds, per (K, mode):
  assign_us       one sc_assign_poses_frame_device call (the memset of the records and the kernel), no d_d2;
  assign_b2b_us   ten such calls between one event pair, per call: the GPU never waits for the host's next enqueue;
  polish_poses_us one sc_polish_poses_device call on the same poses (SEL_NONE, max_iter 16, no mask): the call it would follow;
  peel_us         one sc_peel_device round on a freshly registered frame (median of 5): the round whose claim order FIRST restates.
Two bounds computed from the counts, as times: bytes — 24 n of points in and 4 n of labels out over the measured copy bandwidth
(6.29 TB/s) —, and fma — 13 n K fused multiply-adds over the vector peak (157.3 TFLOP/s = 78.65 T fma/s; plain v_fma_f32 issues at
half of it).  `nearer` names the larger bound, `fraction` is that bound over assign_b2b_us.
The batch form, beside one sc_register_instances_batch_device call (tools/instances_batch_bench.py's scenes: B two-motion problems of
n correspondences, max_instances 4, min_score 4): one sc_assign_poses_batch_device call on that call's records (stride 80, K = 4).
Kernel time from a trace is taken in a run of its own: rocprofv3 --kernel-trace --stats -- python tools/assign_bench.py --repeats 5
--out '' (the kernels are assign_frame_kernel and assign_batch_kernel).
Prints one JSON line per row, then tables; --out receives the text of every --prepend file (the compiler's resource lines, taken
without a GPU), then both.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

COPY_BYTES_PER_S = 6.29e12
FMA_PER_S = 157.3e12 / 2
MAX_INSTANCES, MIN_SCORE, DISTINCT = 4, 4, 32


def pair(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def timed(torch, stream, fn, warmup, repeats):
    return [pair(torch, stream, fn) for it in range(warmup + repeats)][warmup:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--poses", default="2,8,64,1024")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-sizes", default="128,512")
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign.txt"))
    ap.add_argument("--prepend", action="append", default=[])
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    med = lambda v: round(float(np.median(v)), 1)  # noqa: E731
    rows, brows = [], []
    for name in [c for c in a.configs.split(",") if c]:
        cfg, sc = pkg.synth.make_config_scene(name)
        n, kw = cfg.n, dict(cfg.params(), max_triangles=min(cfg.T, 50_000))
        reg = pkg.Registrar(0)
        stream = torch.cuda.Stream(device=dev)
        reg.set_stream(stream.cuda_stream)
        try:
            d_src, d_tgt = torch.from_numpy(sc.src).to(dev), torch.from_numpy(sc.tgt).to(dev)
            d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_label = torch.zeros(n, dtype=torch.int32, device=dev)
            p = pkg.make_params(**kw)
            torch.cuda.synchronize()

            def frame():
                rc, _ = reg.register_device(d_src.data_ptr(), d_tgt.data_ptr(), n, p, d_Rt.data_ptr(), d_mask.data_ptr())
                assert rc == 0, rc
                torch.cuda.synchronize()

            t_peel = []
            for _ in range(2 + 5):
                frame()
                t_peel.append(pair(torch, stream, lambda: reg.peel_device(d_Rt.data_ptr(), d_mask.data_ptr())))
            frame()
            winner = d_Rt.cpu().numpy().copy()
            for K in (int(x) for x in a.poses.split(",")):
                rng = np.random.default_rng(K)
                poses = np.tile(winner, (K, 1)).astype(np.float32)
                poses[:, 9:] += (rng.normal(size=(K, 3)) * 0.1 * cfg.tau).astype(np.float32)
                poses[3::7, 9:] += np.float32(1000.0 * cfg.L)
                d_pose = torch.from_numpy(poses).to(dev)
                d_asg = torch.zeros(K * 32, dtype=torch.uint8, device=dev); d_pol = torch.zeros(K * 64, dtype=torch.uint8, device=dev)
                qp = pkg.make_polish_poses_params(max_iter=16)
                t_pp = timed(torch, stream, lambda: reg.polish_poses_device(qp, d_pose.data_ptr(), 48, K, 0, d_pol.data_ptr(), 0), 2, 8)
                for mode, mname in ((pkg.SC_ASSIGN_BEST, "BEST"), (pkg.SC_ASSIGN_FIRST, "FIRST")):
                    q = pkg.make_assign_params(mode=mode)
                    one = lambda: reg.assign_poses_frame_device(q, d_pose.data_ptr(), 48, K, 0, d_label.data_ptr(), 0, d_asg.data_ptr())  # noqa: E731
                    t_one = timed(torch, stream, one, a.warmup, a.repeats)
                    t_b2b = [t / 10 for t in timed(torch, stream, lambda: [one() for _ in range(10)], a.warmup, a.repeats)]
                    torch.cuda.synchronize()
                    asg = np.frombuffer(d_asg.cpu().numpy().tobytes(), pkg.ASSIGN_RESULT_DTYPE)
                    labelled = int((d_label.cpu().numpy() >= 0).sum())
                    assert int(asg["count"].sum()) == labelled and (asg["status"] == 0).all()
                    b_bytes, b_fma = 28.0 * n / COPY_BYTES_PER_S * 1e6, 13.0 * n * K / FMA_PER_S * 1e6
                    bound = max(b_bytes, b_fma)
                    row = dict(config=name, n=n, K=K, mode=mname, labelled=labelled, assign_us=med(t_one),
                               assign_min_max=[round(min(t_one), 1), round(max(t_one), 1)], assign_b2b_us=med(t_b2b),
                               polish_poses_us=med(t_pp), peel_us=med(t_peel[2:]), bound_bytes_us=round(b_bytes, 3), bound_fma_us=round(b_fma, 3),
                               nearer="fma" if b_fma > b_bytes else "bytes", fraction=round(bound / med(t_b2b), 4))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        finally:
            reg.close()
    # ---- the batch form beside sc_register_instances_batch_device
    if a.batch_sizes and a.batches:
        kw = dict(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05, max_triangles=2000)
        p = pkg.make_params(**kw)
        reg = pkg.Registrar(0)
        stream = torch.cuda.Stream(device=dev)
        reg.set_stream(stream.cuda_stream)
        try:
            for n in (int(x) for x in a.batch_sizes.split(",")):
                scenes = [pkg.synth.make_scene_motions(n, [0.18, 0.12], 1.0, 0.05, 9500 + n + k) for k in range(DISTINCT)]
                for B in (int(x) for x in a.batches.split(",")):
                    src = np.concatenate([scenes[b % DISTINCT].src for b in range(B)]).astype(np.float32)
                    tgt = np.concatenate([scenes[b % DISTINCT].tgt for b in range(B)]).astype(np.float32)
                    d_src, d_tgt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
                    off = (np.arange(B + 1, dtype=np.uint64) * n).astype(np.uint32)
                    d_res = torch.zeros(MAX_INSTANCES * B * 80, dtype=torch.uint8, device=dev)
                    d_label = torch.zeros(B * n, dtype=torch.int32, device=dev); d_lab2 = torch.zeros(B * n, dtype=torch.int32, device=dev)
                    d_nfound = torch.zeros(B, dtype=torch.int32, device=dev)
                    d_asg = torch.zeros(MAX_INSTANCES * B * 32, dtype=torch.uint8, device=dev)
                    torch.cuda.synchronize()
                    t_ins = timed(torch, stream, lambda: reg.register_instances_batch_device(
                        d_src.data_ptr(), d_tgt.data_ptr(), off, p, MAX_INSTANCES, MIN_SCORE, d_res.data_ptr(), d_label.data_ptr(),
                        d_nfound.data_ptr()), 2, max(5, a.repeats // 3))
                    row = dict(n=n, B=B, K=MAX_INSTANCES, instances_us=med(t_ins))
                    for mode, mname in ((pkg.SC_ASSIGN_FIRST, "first"), (pkg.SC_ASSIGN_BEST, "best")):
                        q = pkg.make_assign_params(mode=mode)
                        t = timed(torch, stream, lambda: reg.assign_poses_batch_device(
                            d_src.data_ptr(), d_tgt.data_ptr(), off, p, q, d_res.data_ptr(), 80, MAX_INSTANCES, d_lab2.data_ptr(), d_asg.data_ptr()),
                            a.warmup, a.repeats)
                        row[f"assign_{mname}_us"] = med(t)
                    torch.cuda.synchronize()
                    row["over_instances"] = round(row["assign_best_us"] / row["instances_us"], 4)
                    brows.append(row)
                    print(json.dumps(row), flush=True)
        finally:
            reg.close()
    lines = []
    for path in a.prepend:
        lines += open(path).read().rstrip("\n").split("\n") + [""]
    lines.append("---- tools/assign_bench.py: one sc_assign_poses_frame_device call on a scored frame, K poses")
    lines += [json.dumps(r) for r in rows]
    table = ["", f"{'config':>6} {'n':>6} {'K':>5} {'mode':>5} | {'assign us (min .. max)':>28} {'b2b':>8} {'polish_poses':>13} {'peel':>8} | {'bytes bound':>11} "
                 f"{'fma bound':>10} {'nearer':>6} {'fraction':>9}"]
    for r in rows:
        t = f"{r['assign_us']:.1f} ({r['assign_min_max'][0]:.1f} .. {r['assign_min_max'][1]:.1f})"
        table.append(f"{r['config']:>6} {r['n']:>6} {r['K']:>5} {r['mode']:>5} | {t:>28} {r['assign_b2b_us']:>8.1f} {r['polish_poses_us']:>13.1f} {r['peel_us']:>8.1f} | "
                     f"{r['bound_bytes_us']:>11.3f} {r['bound_fma_us']:>10.3f} {r['nearer']:>6} {r['fraction']:>9.4f}")
    table += ["", "---- one sc_assign_poses_batch_device call beside one sc_register_instances_batch_device call, K = 4 planes"]
    table += [json.dumps(r) for r in brows]
    table += ["", f"{'n':>4} {'B':>5} | {'instances us':>13} {'assign FIRST us':>16} {'assign BEST us':>15} {'assign/instances':>17}"]
    for r in brows:
        table.append(f"{r['n']:>4} {r['B']:>5} | {r['instances_us']:>13.1f} {r['assign_first_us']:>16.1f} {r['assign_best_us']:>15.1f} {r['over_instances']:>17.4f}")
    print("\n".join(table))
    lines += table
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
