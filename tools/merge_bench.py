#!/usr/bin/env python3
"""What finding and folding the duplicates among K poses costs (include/saccot.h, sc_merge_poses), everything resident in HBM.

  python tools/merge_bench.py [--configs C2,C3] [--poses 8,64,1024] [--repeats 30] [--warmup 5] [--batch-sizes 128,512]
                              [--batches 64,1024,4096] [--out profiles/merge.txt] [--prepend FILE ...] [--trace DIR]

The frame form.  Per config (C2: bench.py's shape, n = 5 000; C3: n = 20 000, scored here on one GPU with T = 50 000): the config's
own scene, registered once: the frame every timed call then runs on.  The K poses are tools/assign_bench.py's: the frame's winner
with small seeded translations added (a tenth of tau), every seventh of them a pose far away — so most of the list is ONE motion many
times over, which is what the entry is for.  Device time by a HIP event pair on the context's stream, median of `repeats` after
`warmup`, in microseconds, per K:
  merge_us        one sc_merge_poses_frame_device call (the memset and the three launches), no d_overlap (the table is the workspace's);
  merge_b2b_us    ten such calls between one event pair, per call: the GPU never waits for the host's next enqueue;
  assign_us       one sc_assign_poses_frame_device call (BEST) on the same poses: it runs the same K residual chains per correspondence
                  and so is the yardstick of the support launch.
The bounds of the call's launches, computed from the counts, as times (W = ceil(n / 64) words a bit row):
  support   bytes — 24 n of points in, 8 K W of bit rows out, over the measured copy bandwidth (6.29 TB/s) — and fma — 13 n K fused
            multiply-adds over the vector peak (157.3 TFLOP/s = 78.65 T fma/s; plain v_fma_f32 issues at half of it);
  overlap   popcount — K (K + 1) / 2 pairs x W words x 4 vector operations (two 32-bit ands, two 32-bit popcounts that add as they
            count) over 78.65 T lane operations/s — and bytes — 8 K W of rows in (once from HBM; every further read of a row is an L2
            hit), 4 K^2 of table out;
  decide    bytes — 4 K^2 of table in (the fold reads half of it), 112 K of records in and out.  ONE workgroup: what it takes is
            latency, not bandwidth, and the bound says how little there is to move.
`--trace DIR` adds the launches' own times: DIR holds the kernel trace of a run of its own of this tool WITH THE SAME ARGUMENTS,
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/merge_bench.py ... --out ''
Per kernel the dispatches are taken in time order; a shape's are the next `calls` of them (this tool enqueues the same calls in the
same order every run), of which the warm-up ones are dropped and the median of the rest is reported beside the kernel's bound.
The batch form, beside one sc_assign_poses_batch_device call (BEST) on the same records (tools/instances_batch_bench.py's scenes: B
two-motion problems of n correspondences; the records are one sc_register_instances_batch_device call's, stride 80, K = 4): one
sc_merge_poses_batch_device call.  Its bounds: bytes — 24 n B of points, 80 K B of records in, 68 K B out — and fma — 13 n K B.
Prints one JSON line per row, then tables; --out receives the text of every --prepend file (the compiler's resource lines, taken
without a GPU), then both.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

COPY_BYTES_PER_S = 6.29e12
FMA_PER_S = 157.3e12 / 2  # also the rate of any one-a-lane vector operation
MAX_INSTANCES, MIN_SCORE, DISTINCT = 4, 4, 32
KERNELS = ("merge_support_kernel", "merge_overlap_kernel", "merge_decide_kernel", "merge_batch_kernel")
B2B = 10


def pair(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def timed(torch, stream, fn, warmup, repeats):
    return [pair(torch, stream, fn) for it in range(warmup + repeats)][warmup:]


def us(x):
    return round(x * 1e6, 3)


def frame_bounds(n, K):
    """-> {launch: (bound_us, which)} from the counts alone"""
    W = (n + 63) // 64
    support = {"bytes": (24.0 * n + 8.0 * K * W) / COPY_BYTES_PER_S, "fma": 13.0 * n * K / FMA_PER_S}
    overlap = {"popcount": 4.0 * (K * (K + 1) / 2) * W / FMA_PER_S, "bytes": (8.0 * K * W + 4.0 * K * K) / COPY_BYTES_PER_S}
    decide = {"bytes": (4.0 * K * K + 112.0 * K) / COPY_BYTES_PER_S}
    out = {}
    for name, b in (("support", support), ("overlap", overlap), ("decide", decide)):
        which = max(b, key=b.get)
        out[name] = (us(b[which]), which)
    return out


def trace_durations(folder):
    """kernel -> its dispatches' durations in microseconds, in time order"""
    found = {k: [] for k in KERNELS}
    for f in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            for k in KERNELS:
                if k in row["Kernel_Name"]:
                    found[k].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    return {k: [d for _, d in sorted(v)] for k, v in found.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--poses", default="8,64,1024")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-sizes", default="128,512")
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge.txt"))
    ap.add_argument("--prepend", action="append", default=[])
    ap.add_argument("--trace", default="")
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    med = lambda v: round(float(np.median(v)), 1)  # noqa: E731
    trace = trace_durations(a.trace) if a.trace else None
    taken = {k: 0 for k in KERNELS}

    def traced(kernel, calls, warm):
        """the median of this shape's dispatches of `kernel` (None without a trace, or if the trace is of another run)"""
        if trace is None:
            return None
        mine = trace[kernel][taken[kernel]: taken[kernel] + calls]
        taken[kernel] += calls
        return round(float(np.median(mine[warm:])), 2) if len(mine) == calls else None

    frame_calls = 1 + (a.warmup + a.repeats) * (1 + B2B)  # of sc_merge_poses_frame_device per shape: the check, the singles, the tens
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
            torch.cuda.synchronize()
            rc, _ = reg.register_device(d_src.data_ptr(), d_tgt.data_ptr(), n, pkg.make_params(**kw), d_Rt.data_ptr(), d_mask.data_ptr())
            assert rc == 0, rc
            torch.cuda.synchronize()
            winner = d_Rt.cpu().numpy().copy()
            for K in (int(x) for x in a.poses.split(",")):
                rng = np.random.default_rng(K)
                poses = np.tile(winner, (K, 1)).astype(np.float32)
                poses[:, 9:] += (rng.normal(size=(K, 3)) * 0.1 * cfg.tau).astype(np.float32)
                poses[3::7, 9:] += np.float32(1000.0 * cfg.L)
                d_pose = torch.from_numpy(poses).to(dev)
                d_out = torch.zeros(K * 64, dtype=torch.uint8, device=dev); d_parent = torch.zeros(K, dtype=torch.int32, device=dev)
                d_count = torch.zeros(2, dtype=torch.int32, device=dev); d_asg = torch.zeros(K * 32, dtype=torch.uint8, device=dev)
                mp, q = pkg.make_merge_params(), pkg.make_assign_params()
                one = lambda: reg.merge_poses_frame_device(mp, d_pose.data_ptr(), 48, K, 0, d_out.data_ptr(), d_parent.data_ptr(), 0,  # noqa: E731
                                                           d_count.data_ptr())
                asg = lambda: reg.assign_poses_frame_device(q, d_pose.data_ptr(), 48, K, 0, d_label.data_ptr(), 0, d_asg.data_ptr())  # noqa: E731
                one()
                torch.cuda.synchronize()
                kept, valid = (int(x) for x in d_count.cpu().numpy().view(np.uint32))
                rec = np.frombuffer(d_out.cpu().numpy().tobytes(), pkg.MERGE_POSE_DTYPE)
                assert valid == K and kept == int((rec["status"] == 0).sum()) and (d_parent.cpu().numpy() >= 0).all()
                t_one = timed(torch, stream, one, a.warmup, a.repeats)
                t_b2b = [t / B2B for t in timed(torch, stream, lambda: [one() for _ in range(B2B)], a.warmup, a.repeats)]
                t_asg = timed(torch, stream, asg, a.warmup, a.repeats)
                torch.cuda.synchronize()
                bounds = frame_bounds(n, K)
                row = dict(config=name, n=n, K=K, kept=kept, inliers_max=int(rec["count"].max()), merge_us=med(t_one),
                           merge_min_max=[round(min(t_one), 1), round(max(t_one), 1)], merge_b2b_us=med(t_b2b), assign_us=med(t_asg),
                           over_assign=round(med(t_b2b) / med(t_asg), 3))
                for launch in ("support", "overlap", "decide"):
                    row[f"{launch}_bound_us"], row[f"{launch}_bound"] = bounds[launch]
                    row[f"{launch}_us"] = traced(f"merge_{launch}_kernel", frame_calls, 1 + a.warmup)
                    if row[f"{launch}_us"]:
                        row[f"{launch}_fraction"] = round(bounds[launch][0] / row[f"{launch}_us"], 4)
                rows.append(row)
                print(json.dumps(row), flush=True)
        finally:
            reg.close()
    # ---- the batch form beside sc_assign_poses_batch_device
    if a.batch_sizes and a.batches:
        p = pkg.make_params(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05, max_triangles=2000)
        reg = pkg.Registrar(0)
        stream = torch.cuda.Stream(device=dev)
        reg.set_stream(stream.cuda_stream)
        try:
            for n in (int(x) for x in a.batch_sizes.split(",")):
                scenes = [pkg.synth.make_scene_motions(n, [0.18, 0.12], 1.0, 0.05, 9500 + n + k) for k in range(DISTINCT)]
                for B in (int(x) for x in a.batches.split(",")):
                    K = MAX_INSTANCES
                    src = np.concatenate([scenes[b % DISTINCT].src for b in range(B)]).astype(np.float32)
                    tgt = np.concatenate([scenes[b % DISTINCT].tgt for b in range(B)]).astype(np.float32)
                    d_src, d_tgt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
                    off = (np.arange(B + 1, dtype=np.uint64) * n).astype(np.uint32)
                    d_res = torch.zeros(K * B * 80, dtype=torch.uint8, device=dev)
                    d_label = torch.zeros(B * n, dtype=torch.int32, device=dev); d_nfound = torch.zeros(B, dtype=torch.int32, device=dev)
                    d_asg = torch.zeros(K * B * 32, dtype=torch.uint8, device=dev)
                    d_out = torch.zeros(K * B * 64, dtype=torch.uint8, device=dev); d_parent = torch.zeros(K * B, dtype=torch.int32, device=dev)
                    d_count = torch.zeros(2 * B, dtype=torch.int32, device=dev)
                    torch.cuda.synchronize()
                    reg.register_instances_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, K, MIN_SCORE, d_res.data_ptr(),
                                                        d_label.data_ptr(), d_nfound.data_ptr())
                    torch.cuda.synchronize()
                    mp, q = pkg.make_merge_params(), pkg.make_assign_params()
                    t_mrg = timed(torch, stream, lambda: reg.merge_poses_batch_device(
                        d_src.data_ptr(), d_tgt.data_ptr(), off, p, mp, d_res.data_ptr(), 80, K, d_out.data_ptr(), d_parent.data_ptr(),
                        d_count.data_ptr()), a.warmup, a.repeats)
                    t_asg = timed(torch, stream, lambda: reg.assign_poses_batch_device(
                        d_src.data_ptr(), d_tgt.data_ptr(), off, p, q, d_res.data_ptr(), 80, K, d_label.data_ptr(), d_asg.data_ptr()),
                        a.warmup, a.repeats)
                    torch.cuda.synchronize()
                    cnt = d_count.cpu().numpy().view(np.uint32).reshape(B, 2)
                    b = {"bytes": (24.0 * n * B + 148.0 * K * B) / COPY_BYTES_PER_S, "fma": 13.0 * n * K * B / FMA_PER_S}
                    which = max(b, key=b.get)
                    row = dict(n=n, B=B, K=K, merge_us=med(t_mrg), assign_us=med(t_asg), over_assign=round(med(t_mrg) / med(t_asg), 3),
                               kept_mean=round(float(cnt[:, 0].mean()), 2), valid_mean=round(float(cnt[:, 1].mean()), 2),
                               bound_us=us(b[which]), bound=which, kernel_us=traced("merge_batch_kernel", a.warmup + a.repeats, a.warmup))
                    row["fraction"] = round(row["bound_us"] / (row["kernel_us"] or row["merge_us"]), 4)
                    brows.append(row)
                    print(json.dumps(row), flush=True)
        finally:
            reg.close()
    lines = []
    for path in a.prepend:
        lines += open(path).read().rstrip("\n").split("\n") + [""]
    lines.append("---- tools/merge_bench.py: one sc_merge_poses_frame_device call on a scored frame, K poses"
                 + (" (the launches' own times: a kernel trace taken in a run of its own)" if trace else " (no kernel trace: the launches' own times are not measured)"))
    lines += [json.dumps(r) for r in rows]
    fmt = lambda v: "-" if v is None else f"{v:.2f}"  # noqa: E731
    table = ["", f"{'config':>6} {'n':>6} {'K':>5} {'kept':>5} | {'merge us (min .. max)':>28} {'b2b':>8} {'assign':>8} {'b2b/assign':>10} | "
                 f"{'support us / bound (which)':>32} | {'overlap us / bound (which)':>32} | {'decide us / bound':>22}"]
    for r in rows:
        t = f"{r['merge_us']:.1f} ({r['merge_min_max'][0]:.1f} .. {r['merge_min_max'][1]:.1f})"
        cells = [f"{fmt(r[f'{x}_us'])} / {r[f'{x}_bound_us']:.3f} ({r[f'{x}_bound']})" for x in ("support", "overlap", "decide")]
        table.append(f"{r['config']:>6} {r['n']:>6} {r['K']:>5} {r['kept']:>5} | {t:>28} {r['merge_b2b_us']:>8.1f} {r['assign_us']:>8.1f} {r['over_assign']:>10.3f} | "
                     f"{cells[0]:>32} | {cells[1]:>32} | {cells[2]:>22}")
    table += ["", "---- one sc_merge_poses_batch_device call beside one sc_assign_poses_batch_device call on the same records, K = 4 planes"]
    table += [json.dumps(r) for r in brows]
    table += ["", f"{'n':>4} {'B':>5} | {'merge us':>9} {'kernel us':>10} {'assign us':>10} {'merge/assign':>13} | {'kept':>5} {'valid':>6} | {'bound us':>9} {'which':>6} {'fraction':>9}"]
    for r in brows:
        table.append(f"{r['n']:>4} {r['B']:>5} | {r['merge_us']:>9.1f} {fmt(r['kernel_us']):>10} {r['assign_us']:>10.1f} {r['over_assign']:>13.3f} | "
                     f"{r['kept_mean']:>5.2f} {r['valid_mean']:>6.2f} | {r['bound_us']:>9.3f} {r['bound']:>6} {r['fraction']:>9.4f}")
    print("\n".join(table))
    lines += table
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
